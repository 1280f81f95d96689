"""Image-text retrieval on the MI355X: one JSON line per configuration, in bench.py's style.

  python tools/irtr_bench.py [--what recall step] [--layers 12] [--dtype bf16] [--rounds 7] [--images 8] [--step-batches 4 8]

recall: throughput of the recall evaluation in scored (image, caption) pairs per second at 384 x 384 images and 40-token captions.
  baseline  the reference's schedule with the code this library had before the cached rank pass: one image expanded to 64 copies x 64
            captions through the public infer() on pixels, torch for the score.
  cached    the cached rank pass (visual_embed once per image, objectives.irtr_score_matrix) at 64, 128 and 256 sequences per pass, as
            1 x T tiles (one image x T captions) and as I x T tiles (I images x 64 captions).
  Baseline and candidates alternate inside one process for --rounds rounds; reported: the median ms per pass, the min / max over the
  rounds, pairs per second from the median.  A candidate is "not slower" when its median is within the baseline's own spread.
step: the itm + irtr optimizer step (training_step + backward + fused AdamW, 15 false texts) at per_gpu_batchsize 4 and 8 (64 / 128
  sequences), and csrc/irtr.hip's share of it (score + cross-entropy forward, cross-entropy gradient + backward, timed with events)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_pkg  # noqa: F401,E402
from rmcl_amd.vilt.config import task_finetune_irtr_coco, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, objectives  # noqa: E402


def text_of(n, cfg, dev, seed):
    g = torch.Generator().manual_seed(seed)
    L = cfg["max_text_len"]
    ids = torch.randint(1000, cfg["vocab_size"], (n, L), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    return ids.to(dev), torch.ones(n, L, dtype=torch.int64, device=dev)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def run_recall(a, dev):
    cfg = task_finetune_irtr_coco(num_layers=a.layers, per_gpu_batchsize=64, drop_rate=0.0, max_steps=10, get_recall_metric=False,
                                  dense_images=True)
    m = ViLTransformerSS(cfg, device=dev, compute_dtype=a.dtype)
    m.eval()
    eng = m.engine
    S = cfg["image_size"]
    g = torch.Generator().manual_seed(1)
    images = (torch.rand(a.images, 3, S, S, generator=g) * 2 - 1).to(dev)
    ids, msk = text_of(256, cfg, dev, 2)
    with torch.no_grad():
        emb, imk, _, _ = m.visual_embed(images)
    embeds, masks = emb.contiguous(), imk.to(torch.int32).contiguous()
    counts = [emb.shape[1] - 1] * a.images
    w, b = eng.rank_params()

    def baseline():                                                   # one image x 64 captions, pixels expanded, the public infer
        with torch.no_grad():
            out = m.infer({"image": [images[:1].expand(64, -1, -1, -1)], "text_ids": ids[:64], "text_masks": msk[:64]})
            return out["cls_feats"] @ w + b

    def cached(I, T):
        def f():
            objectives.irtr_score_matrix(m, embeds[:I], masks[:I], counts[:I], ids[:T], msk[:T], I, T)
        return f

    cands = [("baseline_infer_1x64", 64, baseline), ("cached_1x64", 64, cached(1, 64)), ("cached_1x128", 128, cached(1, 128)),
             ("cached_1x256", 256, cached(1, 256)), ("cached_2x64", 128, cached(2, 64)), ("cached_4x64", 256, cached(4, 64))]
    for _, _, f in cands:                                             # warm every shape
        for _ in range(3):
            f()
    res = {n: [] for n, _, _ in cands}
    for _ in range(a.rounds):
        for n, _, f in cands:                                         # alternate inside one process
            res[n].append(timed(f, a.reps))
    base = res["baseline_infer_1x64"]
    bmed, bspread = statistics.median(base), max(base) - min(base)
    for n, pairs, _ in cands:
        med = statistics.median(res[n])
        print(json.dumps({"metric": "irtr_recall_pairs_per_s", "config": n, "pairs_per_pass": pairs, "layers": a.layers, "dtype": a.dtype,
                          "ms_per_pass_median": round(med, 4), "ms_min": round(min(res[n]), 4), "ms_max": round(max(res[n]), 4),
                          "pairs_per_s": round(pairs / med * 1e3, 1), "rounds": a.rounds, "reps": a.reps,
                          "ms_per_pair_vs_baseline": round((med / pairs) / (bmed / 64), 4),
                          "not_slower_than_baseline_within_its_spread": bool(med / pairs * 64 <= bmed + bspread)}), flush=True)
    t = timed(lambda: m.visual_embed(images[:1]), 20)
    print(json.dumps({"metric": "irtr_visual_embed_ms_per_image", "dtype": a.dtype, "ms": round(t, 4)}), flush=True)


def run_step(a, B, dev):
    cfg = task_finetune_irtr_coco(num_layers=a.layers, per_gpu_batchsize=B, max_steps=10 ** 6, warmup_steps=0, dense_images=True,
                                  get_recall_metric=False, loss_names=_loss_names({"itm": 1, "irtr": 1}))
    m = ViLTransformerSS(cfg, device=dev, compute_dtype=a.dtype)
    (opt,), _ = m.configure_optimizers()
    m.train()
    S, Fn = cfg["image_size"], cfg["draw_false_text"]
    g = torch.Generator().manual_seed(3)
    img = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    ids, msk = text_of(B, cfg, dev, 4)
    batch = {"image": [img], "false_image_0": [torch.roll(img, 1, 0)], "text": ["x"] * B, "text_ids": ids, "text_masks": msk}
    for i in range(Fn):
        batch[f"false_text_{i}_ids"], batch[f"false_text_{i}_masks"] = text_of(B, cfg, dev, 10 + i)
    times, loss = [], None
    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.zero_grad()
        loss = m.training_step(batch, i)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    eng = m.engine
    Sq, R, D = B * (Fn + 1), Fn + 1, cfg["hidden_size"]
    cls = torch.randn(Sq, D, device=dev)
    scores, dscore, dcls = torch.empty(Sq, device=dev), torch.empty(Sq, device=dev), torch.empty(Sq, D, device=dev)
    one = torch.ones(1, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fw, bw = [], []
    for i in range(30):
        ev[0].record()
        eng.irtr_score(cls, scores)
        eng.irtr_ce(scores, B, R, 1.0)
        ev[1].record()
        eng.irtr_ce(scores, B, R, 1.0, dscore=dscore, scale_dev=one)
        eng.irtr_backward(dscore, cls, dcls, with_grads=True)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= 5:
            fw.append(ev[0].elapsed_time(ev[1]))
            bw.append(ev[1].elapsed_time(ev[2]))
    med = statistics.median(times)
    kf, kb = statistics.median(fw), statistics.median(bw)
    print(json.dumps({"metric": "irtr_finetune_step_ms", "tasks": "itm+irtr", "per_gpu_batchsize": B, "sequences": Sq, "layers": a.layers,
                      "dtype": a.dtype, "ms_per_step_median": round(med, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                      "images_per_s": round(B / med * 1e3, 1), "irtr_hip_fwd_ms": round(kf, 4), "irtr_hip_bwd_ms": round(kb, 4),
                      "irtr_hip_share_of_step": round((kf + kb) / med, 5), "loss": float(loss)}), flush=True)
    del m, opt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["recall", "step"])
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-batches", type=int, nargs="+", default=[4, 8])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/irtr_bench.py measures on the GPU; no device found")
    if "recall" in a.what:
        run_recall(a, "cuda:0")
    if "step" in a.what:
        for B in a.step_batches:
            run_step(a, B, "cuda:0")


if __name__ == "__main__":
    main()
