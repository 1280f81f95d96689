"""Streaming attention against the unfused path on the MI355X: one JSON line per shape, in bench.py's style.

  python tools/attention_stream_bench.py [--what kernels step] [--rounds 7] [--reps 50] [--out FILE]

kernels: forward + backward of masked multi-head self-attention at B = 64, H = 12, N = 281 (384 x 640 images: 240 + 1 + 40 tokens) and
  N = 512, bf16, unit-normal qkv / dout, the text-pad + image-pad mask of a real batch.
  unfused   rmcl_attention_fwd / rmcl_attention_bwd (bf16, exact = 0): score GEMM, softmax kernels, [B, H, N, ldp] probabilities in HBM.
  stream    rmcl_attention_stream_fwd / rmcl_attention_stream_bwd on the same buffers.
  Both in one process, alternating, for --rounds rounds of --reps forward + backward pairs timed by device events; reported: the median ms per pair, min / max over
  the rounds, and the ratio of the medians.  "not slower" means the streaming median is at most the unfused median.
step: one attacked VQA step (K = adv_steps_img of the task config, 12 layers) at per_gpu_batchsize 128 on a batch of 384 x 640 images:
  the bf16 engine with long_sequences against the fp32 engine (which has no token limit) - a first measurement of the workload."""
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
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P  # noqa: E402
from rmcl_amd.runtime import stream_ptr  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    """ms per call from device events around `reps` back-to-back calls on the current stream (host launch cost stays out of the figure
    as long as the queue is ahead of the device; a warm call in front fills it)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_kernels(a, N, B=64, H=12):
    D = H * 64
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B * N, 3 * D, generator=g).to(DEV, torch.bfloat16)
    dout = torch.randn(B * N, D, generator=g).to(DEV, torch.bfloat16)
    mask = torch.ones(B, N, dtype=torch.int32)
    for b in range(B):
        mask[b, (8, 39, 23)[b % 3]:40] = 0
        tail = (13, 5, 0)[b % 3]
        if tail:
            mask[b, N - tail:] = 0
    mask = mask.to(DEV)
    ne = int(lib.rmcl_attention_scratch_elems(B, H, N))
    out = torch.empty(B * N, D, dtype=torch.bfloat16, device=DEV)
    dqkv = torch.empty(B * N, 3 * D, dtype=torch.bfloat16, device=DEV)
    probs = torch.empty(ne, dtype=torch.bfloat16, device=DEV)
    scores = torch.empty(ne, dtype=torch.float32, device=DEV)
    dS = torch.empty(ne, dtype=torch.bfloat16, device=DEV)

    def unfused():
        check(lib.rmcl_attention_fwd(P(qkv), P(mask), P(out), P(probs), P(scores), B, N, H, L.BF16, 0, stream_ptr()), "attention_fwd")
        check(lib.rmcl_attention_bwd(P(qkv), P(mask), P(probs), P(dout), P(out), P(dqkv), P(scores), P(dS), B, N, H, L.BF16, 0, stream_ptr()),
              "attention_bwd")

    def stream():
        check(lib.rmcl_attention_stream_fwd(P(qkv), P(mask), P(out), P(probs), P(scores), B, N, H, stream_ptr()), "attention_stream_fwd")
        check(lib.rmcl_attention_stream_bwd(P(qkv), P(mask), P(probs), P(dout), P(out), P(dqkv), P(scores), P(dS), B, N, H, stream_ptr()),
              "attention_stream_bwd")

    def stream_fwd():
        check(lib.rmcl_attention_stream_fwd(P(qkv), P(mask), P(out), P(probs), P(scores), B, N, H, stream_ptr()), "attention_stream_fwd")

    def unfused_fwd():
        check(lib.rmcl_attention_fwd(P(qkv), P(mask), P(out), P(probs), P(scores), B, N, H, L.BF16, 0, stream_ptr()), "attention_fwd")

    cands = [("unfused", unfused), ("stream", stream), ("unfused_fwd", unfused_fwd), ("stream_fwd", stream_fwd)]
    for _, f in cands:
        for _ in range(3):
            f()
    res = {n: [] for n, _ in cands}
    for _ in range(a.rounds):
        for n, f in cands:                                            # alternate inside one process
            res[n].append(timed(f, a.reps))
    med = {n: statistics.median(v) for n, v in res.items()}
    rec = {"metric": "attention_fwd_bwd_ms", "B": B, "H": H, "N": N, "dtype": "bf16", "rounds": a.rounds, "reps": a.reps,
           "hbm_bytes_unfused_matrices": 2 * ne * 2 + 2 * ne * 4}
    for n in res:
        rec[n] = {"ms_median": round(med[n], 4), "ms_min": round(min(res[n]), 4), "ms_max": round(max(res[n]), 4)}
    rec["stream_over_unfused"] = round(med["stream"] / med["unfused"], 4)
    rec["stream_fwd_over_unfused_fwd"] = round(med["stream_fwd"] / med["unfused_fwd"], 4)
    rec["stream_not_slower"] = bool(med["stream"] <= med["unfused"])
    return rec


def run_step(a):
    from rmcl_amd.vilt.config import task_finetune_vqa_randaug_attacked
    from rmcl_amd.vilt.modules import ViLTransformerSS
    B = a.step_batch
    out = {"metric": "vqa_attacked_step_ms", "per_gpu_batchsize": B, "image": "384x640", "tokens": 281, "layers": a.layers,
           "note": "first measurement"}
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(B, 3, 384, 640, generator=g) * 2 - 1)
    ids = torch.randint(1000, 30000, (B, 40), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    labels = [[int(x) for x in torch.randint(0, 3129, (3,), generator=g)] for _ in range(B)]
    scores = [[1.0, 0.6, 0.3] for _ in range(B)]
    for dtype, over in (("bf16", {"long_sequences": True}), ("f32", {})):
        cfg = task_finetune_vqa_randaug_attacked(image_view=True, num_layers=a.layers, per_gpu_batchsize=B, max_steps=10 ** 6, warmup_steps=0,
                                                 **over)
        m = ViLTransformerSS(cfg, device=DEV, compute_dtype=dtype)
        (opt,), _ = m.configure_optimizers()
        m.train()
        batch = {"image": [img.to(DEV)], "text": ["x"] * B, "text_ids": ids.to(DEV), "text_masks": torch.ones(B, 40, dtype=torch.int64, device=DEV),
                 "vqa_labels": labels, "vqa_scores": scores}
        times, loss = [], None
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.zero_grad()
            loss = m.training_step(dict(batch, image=[batch["image"][0]]), i)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(times)
        out[dtype] = {"ms_per_step_median": round(med, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                      "images_per_s": round(B / med * 1e3, 1), "adv_steps_img": int(cfg["adv_steps_img"]), "loss": float(loss)}
        del m, opt
        torch.cuda.empty_cache()
    out["bf16_long_sequences_over_f32"] = round(out["bf16"]["ms_per_step_median"] / out["f32"]["ms_per_step_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["kernels", "step"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--step-batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/attention_stream_bench.py measures on the GPU; no device found")
    if a.rounds < 7:
        raise SystemExit("--rounds: at least 7")
    recs = []
    if "kernels" in a.what:
        for N in (281, 512):
            recs.append(run_kernels(a, N))
            print(json.dumps(recs[-1]), flush=True)
    if "step" in a.what:
        recs.append(run_step(a))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/attention_stream_bench.py", "device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
