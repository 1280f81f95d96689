"""Masked-patch-prediction pre-training step on the MI355X: JSON lines in bench.py's style, appended to --out.

  python tools/mpp_bench.py --bs 64 --steps 20 --warmup 5 [--layers 12] [--dtype bf16] [--out profiles/mpp_bench.jsonl] [--commit ID]

(a) ms per optimizer step of the `mpp` task alone and (b) of `mlm + itm + mpp` (training_step + backward + fused AdamW), per-step device
events, medians; (c) the head alone at the same shape: the compacted path (gather, transform, decoder, three cross-entropies,
backward with all weight gradients, scatter; the bind - labels, mask gather, compaction - is timed apart) against the reference's
schedule - the same head on ALL B (1 + P) image rows in torch (bf16 autocast linear layers, fp32 cross_entropy with ignore_index over
[B (1 + P) 3, 256], autograd backward) - and, forward only, against this library's own all-rows listing (the dense-logits pass).  The
variants alternate inside one process; medians.  Nothing here is a pass criterion: the comparison figure is the all-rows baseline of the same run.

  python tools/mpp_bench.py --u8 [--bs 64] [--steps 20] [--head-iters 20] [--out profiles/mpp_u8_bench.json]

The byte feed: (d) stream time of rmcl_mpp_labels_u8 on a Uint8Batch against rmcl_mpp_labels on its float image (B x 384 x 384, dense
form), alternating in one process, medians; (e) the `mpp` and `mlm + itm + mpp` steps fed the Uint8Batch against the same steps of the same
model fed the float batch, alternating step by step.  One JSON object, written to --out."""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_pkg  # noqa: F401,E402
from rmcl_amd.vilt.config import task_mlm_itm_mpp, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from rmcl_amd.vilt.modules.objectives import mpp_image_labels  # noqa: E402
from tools.mlm_bench import batch_of, clocks, median  # noqa: E402


def time_steps(tasks, a, dev):
    cfg = task_mlm_itm_mpp(num_layers=a.layers, per_gpu_batchsize=a.bs, max_steps=10 ** 6, warmup_steps=0, dense_images=True,
                           loss_names=_loss_names(tasks))
    m = ViLTransformerSS(cfg, device=dev, compute_dtype=a.dtype)
    (opt,), _ = m.configure_optimizers()
    m.train()
    batch = batch_of(a.bs, cfg, dev)
    ms, loss = [], None
    for i in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.zero_grad()
        loss = m.training_step(batch, i)
        loss.backward()
        opt.step()
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    P = (cfg["image_size"] // cfg["patch_size"]) ** 2
    return m, cfg, batch, median(ms), min(ms), max(ms), float(m.logged["mpp/train/loss"]), int(m.engine.mpp_bufs(a.bs, "mpp", P).count[0])


def head_alone(m, cfg, batch, a, dev):
    from rmcl_amd.runtime import mpp_draw_masks
    eng = m.engine
    B, Lt, D = a.bs, cfg["max_text_len"], cfg["hidden_size"]
    P = (cfg["image_size"] // cfg["patch_size"]) ** 2
    N = Lt + 1 + P
    xn = torch.randn(B * N, D, device=dev)
    img = batch["image"][0].float().contiguous()
    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], img, tag="bench")
    mp = eng.mpp_bufs(B, "bench", P)
    torch.manual_seed(0)
    masked, replaced = mpp_draw_masks(B, P)
    one = torch.ones(1, device=dev)
    dxn = torch.zeros(B * N, D, device=dev)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items() if k.startswith("mpp_score.")}
    eng.mpp_bind(mp, img, pb, masked, replaced)
    labels = mpp_image_labels(mp)                                           # [B, 1 + P, 3]
    feats = xn.view(B, N, D)[:, Lt:].detach().clone().requires_grad_(True)
    F = torch.nn.functional

    ma = eng.mpp_bufs(B, "bench_dense", P)
    eng.mpp_bind(ma, img, pb, masked, replaced, all_rows=True)

    def bind():
        eng.mpp_bind(mp, img, pb, masked, replaced)

    def compacted():
        eng.mpp_forward(mp, xn)
        eng.mpp_backward(mp, 1.0, one, dxn, with_grads=True)

    def all_rows():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = F.linear(feats, sd["mpp_score.transform.dense.weight"], sd["mpp_score.transform.dense.bias"])
            h = F.layer_norm(F.gelu(h), (D,), sd["mpp_score.transform.LayerNorm.weight"], sd["mpp_score.transform.LayerNorm.bias"], 1e-12)
            z = F.linear(h, sd["mpp_score.decoder.weight"], sd["mpp_score.decoder.bias"])
        loss = F.cross_entropy(z.float().view(-1, 256), labels.view(-1), ignore_index=-100)
        return torch.autograd.grad(loss, [feats] + list(sd.values()))

    t = {k: [] for k in ("bind", "compacted", "all_rows", "fwd_compacted", "fwd_all_rows_native")}
    fns = {"bind": bind, "compacted": compacted, "all_rows": all_rows, "fwd_compacted": lambda: eng.mpp_forward(mp, xn),
           "fwd_all_rows_native": lambda: eng.mpp_forward(ma, xn)}
    for i in range(a.head_iters + 5):
        ev = {}
        for k, fn in fns.items():
            ev[k] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[k][0].record(); fn(); ev[k][1].record()
        torch.cuda.synchronize()
        if i >= 5:
            for k in t:
                t[k].append(ev[k][0].elapsed_time(ev[k][1]))
    return {"bind_ms": round(median(t["bind"]), 4), "compacted_head_ms": round(median(t["compacted"]), 4),
            "compacted_head_ms_min": round(min(t["compacted"]), 4), "all_rows_head_ms": round(median(t["all_rows"]), 4),
            "all_rows_head_ms_min": round(min(t["all_rows"]), 4), "compacted_forward_ms": round(median(t["fwd_compacted"]), 4),
            "all_rows_native_forward_ms": round(median(t["fwd_all_rows_native"]), 4), "masked_rows": int(mp.count[0]), "launch_rows": mp.rows,
            "all_rows": B * (P + 1)}


def byte_feed(a, dev):
    from rmcl_amd._lib import lib, check, P
    from rmcl_amd.runtime import stream_ptr
    from rmcl_amd.vilt.datasets import Uint8Batch
    from rmcl_amd.vilt.transforms import normalize_lut
    B, S = a.bs, 384
    g = torch.Generator().manual_seed(1)
    u8 = Uint8Batch(torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev), torch.full((B, 2), S, dtype=torch.int32))
    img = u8.float_image().contiguous()
    sizes, lut = u8.sizes.to(dev), normalize_lut().to(dev)
    Pn = (S // 32) ** 2
    lab_f = torch.empty(B, Pn, 3, dtype=torch.int32, device=dev)
    lab_b = torch.empty_like(lab_f)
    fns = {"labels_f32": lambda: check(lib.rmcl_mpp_labels(P(img), B, S, S, None, None, 0, S // 32, Pn, P(lab_f), stream_ptr())),
           "labels_u8": lambda: check(lib.rmcl_mpp_labels_u8(P(u8.data), P(sizes), B, S, S, P(lut), None, None, 0, S // 32, Pn, P(lab_b), stream_ptr()))}
    t = {k: [] for k in fns}
    for i in range(a.head_iters + 5):
        ev = {}
        for k, fn in fns.items():
            ev[k] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[k][0].record(); fn(); ev[k][1].record()
        torch.cuda.synchronize()
        if i >= 5:
            for k in t:
                t[k].append(ev[k][0].elapsed_time(ev[k][1]))
    out = {"labels_equal": bool(torch.equal(lab_f, lab_b)), "labels_repeats": a.head_iters,
           "labels_f32_ms": round(median(t["labels_f32"]), 4), "labels_f32_ms_min": round(min(t["labels_f32"]), 4),
           "labels_u8_ms": round(median(t["labels_u8"]), 4), "labels_u8_ms_min": round(min(t["labels_u8"]), 4)}
    for name, tasks in (("mpp", {"mpp": 1}), ("mlm+itm+mpp", {"mlm": 1, "itm": 1, "mpp": 1})):
        cfg = task_mlm_itm_mpp(num_layers=a.layers, per_gpu_batchsize=B, max_steps=10 ** 6, warmup_steps=0, loss_names=_loss_names(tasks))
        m = ViLTransformerSS(cfg, device=dev, compute_dtype=a.dtype)
        (opt,), _ = m.configure_optimizers()
        m.train()
        base = batch_of(B, cfg, dev)
        u8f = Uint8Batch(torch.roll(u8.data, 1, 0).contiguous(), u8.sizes)
        feeds = {"float": dict(base, image=[img], false_image_0=[u8f.float_image().contiguous()]), "bytes": dict(base, image=[u8], false_image_0=[u8f])}
        ms = {k: [] for k in feeds}
        for i in range(a.warmup + a.steps):
            for k, batch in feeds.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m.zero_grad()
                loss = m.training_step(dict(batch), i)
                loss.backward()
                opt.step()
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        out[name] = {"steps": a.steps, "float_ms_per_step": round(median(ms["float"]), 3), "float_ms_min": round(min(ms["float"]), 3),
                     "bytes_ms_per_step": round(median(ms["bytes"]), 3), "bytes_ms_min": round(min(ms["bytes"]), 3)}
        del m, opt
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--head-iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None, help="default: profiles/mpp_bench.jsonl (appended), with --u8 profiles/mpp_u8_bench.json (written)")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--u8", action="store_true", help="the byte feed against the float feed (labels kernel and steps); one JSON object to --out")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "mpp_u8_bench.json" if a.u8 else "mpp_bench.jsonl")
    dev = "cuda:0"
    prop = torch.cuda.get_device_properties(0)
    env = {"box": socket.gethostname(), "device": prop.name, "clocks": clocks(), "cus": prop.multi_processor_count,
           "commit": a.commit, "bs": a.bs, "layers": a.layers, "dtype": a.dtype, "text_len": 40, "image": 384, "mask_prob": 0.15}
    if a.u8:
        rec = dict(env, metric="mpp_u8_feed", **byte_feed(a, dev))
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        return
    lines = []
    m, cfg, batch, med, lo, hi, loss, n = time_steps({"mpp": 1}, a, dev)
    lines.append(dict(env, metric="mpp_step_ms", task="mpp", ms_per_step=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                      samples_per_s=round(a.bs / med * 1e3, 1), mpp_loss=loss, masked_rows=n))
    lines.append(dict(env, metric="mpp_head_ms", **head_alone(m, cfg, batch, a, dev)))
    del m
    torch.cuda.empty_cache()
    m, cfg, batch, med, lo, hi, loss, n = time_steps({"mlm": 1, "itm": 1, "mpp": 1}, a, dev)
    lines.append(dict(env, metric="mpp_step_ms", task="mlm+itm+mpp", ms_per_step=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                      samples_per_s=round(a.bs / med * 1e3, 1), mpp_loss=loss, masked_rows=n))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
