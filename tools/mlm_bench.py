"""Masked-language-modelling pre-training step on the MI355X: JSON lines in bench.py's style, appended to --out.

  python tools/mlm_bench.py --bs 64 --steps 20 --warmup 5 [--layers 12] [--dtype bf16] [--out profiles/mlm_bench.jsonl] [--commit ID]

(a) ms per optimizer step of the `mlm` task alone and (b) of `mlm + itm` (training_step + backward + fused AdamW), per-step device
events, medians; (c) the head alone at the same shape: the fused path on the compacted masked rows (compaction, gather, transform,
fused decoder + cross-entropy, recomputing backward with all weight gradients, scatter) against a DENSE baseline assembled from the
kernels the library had before this head - rmcl_gemm for the [B L, D] x [D, V] logits (bf16 operands, fp32 logits, vocabulary padded to
a multiple of 128 so the fast GEMM kernels take it), torch's cross_entropy with autograd on the logits, rmcl_gemm for the two backward
products and a column sum for the bias - which is what a straight port of the reference's compute_mlm does.  The dense baseline does
NOT include the transform, the fused path does (on the compacted rows): the comparison is conservative.  A and B alternate inside one
process; medians."""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_pkg  # noqa: F401,E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P, I64, F  # noqa: E402
from rmcl_amd.runtime import stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_mlm_itm, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402


def batch_of(B, cfg, dev, seed=0, mlm_prob=0.15):
    g = torch.Generator().manual_seed(seed)
    Lt, V = cfg["max_text_len"], cfg["vocab_size"]
    ids = torch.randint(1000, V, (B, Lt), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    img = torch.rand(B, 3, cfg["image_size"], cfg["image_size"], generator=g) * 2 - 1
    chosen = torch.rand(B, Lt, generator=g) < mlm_prob
    chosen[:, 0] = chosen[:, -1] = False
    kind = torch.rand(B, Lt, generator=g)
    labels = torch.where(chosen, ids, torch.full_like(ids, -100))
    mlm = ids.clone()
    mlm[chosen & (kind < 0.8)] = 103
    swap = chosen & (kind >= 0.8) & (kind < 0.9)
    mlm[swap] = torch.randint(0, V, (int(swap.sum()),), generator=g)
    # labels stay on the host, as a DataLoader delivers them: the step validates and counts them there without a device read-back
    return {"image": [img.to(dev)], "false_image_0": [torch.roll(img, 1, 0).to(dev)], "text": ["x"] * B, "text_ids": ids.to(dev),
            "text_masks": torch.ones(B, Lt, dtype=torch.int64, device=dev), "text_labels": torch.full((B, Lt), -100),
            "text_ids_mlm": mlm.to(dev), "text_labels_mlm": labels}


def clocks():
    """current (starred) level of the first GPU's shader and memory clock tables, read-only; None where the driver does not show them"""
    import glob
    out = {}
    for key, fn in (("sclk", "pp_dpm_sclk"), ("mclk", "pp_dpm_mclk")):
        out[key] = None
        for path in sorted(glob.glob(f"/sys/class/drm/card*/device/{fn}")):
            try:
                cur = [ln.split()[1] for ln in open(path).read().splitlines() if ln.strip().endswith("*")]
            except OSError:
                continue
            if cur:
                out[key] = cur[0]
                break
    return out


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def time_steps(tasks, a, dev):
    cfg = task_mlm_itm(num_layers=a.layers, per_gpu_batchsize=a.bs, max_steps=10 ** 6, warmup_steps=0, dense_images=True,
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
    return m, cfg, batch, median(ms), min(ms), max(ms), float(m.logged["mlm/train/loss"]), int(m.engine.mlm_bufs(a.bs, "mlm").count)


def head_alone(m, cfg, batch, a, dev):
    eng = m.engine
    B, Lt, D, V = a.bs, cfg["max_text_len"], cfg["hidden_size"], cfg["vocab_size"]
    N = Lt + 1 + (cfg["image_size"] // cfg["patch_size"]) ** 2
    M = B * Lt
    Vp = (V + 127) // 128 * 128
    xn = torch.randn(B * N, D, device=dev)
    mb = eng.mlm_bufs(B, "bench")
    one = torch.ones(1, device=dev)
    dxn = torch.zeros(B * N, D, device=dev)
    # dense baseline operands: h of every text row in bf16, the padded bf16 decoder weight, fp32 logits
    h = torch.randn(M, D, device=dev).to(torch.bfloat16)
    Wp = torch.zeros(Vp, D, dtype=torch.bfloat16, device=dev)
    Wp[:V] = eng.view(eng.q32, eng.mlm.dw, (V, D)).to(torch.bfloat16)
    bias = torch.zeros(Vp, device=dev)
    logits = torch.empty(M, Vp, device=dev)
    dh = torch.empty(M, D, device=dev)
    dW = torch.zeros(Vp, D, device=dev)
    lab = batch["text_labels_mlm"].to(dev).view(-1)
    st = stream_ptr
    route = int(lib.rmcl_gemm_route(M, Vp, D, L.EPI_BIAS, L.F32, 1, 1))

    def fused():
        eng.mlm_bind(mb, batch["text_labels_mlm"], N)
        eng.mlm_forward(mb, xn)
        eng.mlm_backward(mb, 1.0, one, dxn, with_grads=True)

    def dense():
        check(lib.rmcl_gemm(P(h), P(Wp), P(logits), None, P(bias), None, M, Vp, D, I64(D), I64(D), Vp, 0, F(1.0), L.EPI_BIAS, 1, L.BF16, L.F32,
                            1, 1, 0, st()), "dense logits")
        z = logits[:, :V].detach().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(z, lab, ignore_index=-100)
        (dz,) = torch.autograd.grad(loss, z)
        dzp = torch.zeros(M, Vp, dtype=torch.bfloat16, device=dev)
        dzp[:, :V] = dz
        check(lib.rmcl_gemm(P(dzp), P(Wp), P(dh), None, None, None, M, D, Vp, I64(Vp), I64(D), D, 0, F(1.0), 0, 1, L.BF16, L.F32, 1, 0, 0, st()),
              "dense dh")
        check(lib.rmcl_gemm(P(dzp), P(h), P(dW), None, None, None, Vp, D, M, I64(Vp), I64(D), D, 0, F(1.0), L.EPI_ACCUM, 1, L.BF16, L.F32, 0, 0, 0,
                            st()), "dense dW")
        return dz.sum(dim=0)

    tf, td = [], []
    for i in range(a.head_iters + 5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(); fused(); ev[1].record()
        ev[2].record(); dense(); ev[3].record()
        torch.cuda.synchronize()
        if i >= 5:
            tf.append(ev[0].elapsed_time(ev[1]))
            td.append(ev[2].elapsed_time(ev[3]))
    return {"fused_head_ms": round(median(tf), 4), "fused_head_ms_min": round(min(tf), 4), "dense_head_ms": round(median(td), 4),
            "dense_head_ms_min": round(min(td), 4), "masked_rows": int(mb.count), "launch_rows": mb.rows, "dense_rows": M,
            "dense_logits_gemm_route": route}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--head-iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlm_bench.jsonl"))
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    dev = "cuda:0"
    prop = torch.cuda.get_device_properties(0)
    env = {"box": socket.gethostname(), "device": prop.name, "clocks": clocks(), "cus": prop.multi_processor_count,
           "commit": a.commit, "bs": a.bs, "layers": a.layers, "dtype": a.dtype, "text_len": 40, "mlm_prob": 0.15}
    lines = []
    m, cfg, batch, med, lo, hi, loss, n = time_steps({"mlm": 1}, a, dev)
    lines.append(dict(env, metric="mlm_step_ms", task="mlm", ms_per_step=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                      samples_per_s=round(a.bs / med * 1e3, 1), mlm_loss=loss, masked_rows=n))
    lines.append(dict(env, metric="mlm_head_ms", **head_alone(m, cfg, batch, a, dev)))
    del m
    torch.cuda.empty_cache()
    m, cfg, batch, med, lo, hi, loss, n = time_steps({"mlm": 1, "itm": 1}, a, dev)
    lines.append(dict(env, metric="mlm_step_ms", task="mlm+itm", ms_per_step=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                      samples_per_s=round(a.bs / med * 1e3, 1), mlm_loss=loss, masked_rows=n))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
