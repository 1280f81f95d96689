"""What the prediction API costs.

Kernel   stream time (device events around ITERS calls, medians over ROUNDS rounds that alternate the arms in one process) of
         Engine.rows_topk next to its torch restatement (softmax / sigmoid over the whole matrix, then topk) at
             mlm        [2560, 30522] fp32, k = 5, softmax     the dense logits of 64 sentences x 40 positions
             vqa        [256, 3129] at the head's pitch 3136, k = 5, sigmoid
             irtr_rows  [1000, 5000], k = 10, raw              per image its captions
             irtr_cols  the same matrix, per caption its images: the transposed contiguous copy is made inside the timed call, by both arms
         The torch arm of the raw case is topk alone.  Bytes: every arm reads the matrix once at least; achieved GB/s = matrix bytes / time.
Loop     Predictor.fill_mask end to end (12 layers, bf16, 384 x 384 images, wall time between device synchronisations, the final read-back
         included): B = 1 with 5 masks (5 rounds) and B = 64 with 5 masks each.

  python tools/predict_bench.py --out profiles/predict_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS, ROUNDS, WARMUP = 10, 20, 3
LOOP_ROUNDS = 20


def bench_kernels(eng):
    import torch
    dev = eng.device
    g = torch.Generator(device="cpu").manual_seed(0)
    mlm = (torch.randn(2560, 30522, generator=g) * 3).to(dev)
    vqa_p = torch.zeros(256, 3136, device=dev)
    vqa_p[:, :3129] = torch.randn(256, 3129, generator=g).to(dev) * 3
    vqa = vqa_p[:, :3129]
    irtr = torch.randn(1000, 5000, generator=g).to(dev)
    arms = {
        "mlm_rows_topk": lambda: eng.rows_topk(mlm, 5, "softmax"),
        "mlm_torch": lambda: torch.softmax(mlm, dim=1).topk(5, dim=1),
        "vqa_rows_topk": lambda: eng.rows_topk(vqa, 5, "sigmoid"),
        "vqa_torch": lambda: torch.sigmoid(vqa).topk(5, dim=1),
        "irtr_rows_rows_topk": lambda: eng.rows_topk(irtr, 10),
        "irtr_rows_torch": lambda: irtr.topk(10, dim=1),
        "irtr_cols_rows_topk": lambda: eng.rows_topk(irtr.t().contiguous(), 10),
        "irtr_cols_torch": lambda: irtr.t().contiguous().topk(10, dim=1),
    }
    nbytes = {"mlm": mlm.numel() * 4, "vqa": vqa.numel() * 4, "irtr_rows": irtr.numel() * 4, "irtr_cols": irtr.numel() * 4}
    # the kernel's columns are torch.topk's on the raw values (continuous random inputs: no ties) before anything is timed; the torch arms
    # rank the probabilities, which can tie in fp32 where the logits do not (sigmoid near 1)
    for a, x, k in (("mlm_rows_topk", mlm, 5), ("vqa_rows_topk", vqa, 5), ("irtr_rows_rows_topk", irtr, 10), ("irtr_cols_rows_topk", irtr.t(), 10)):
        assert torch.equal(arms[a]()[0].to(torch.int64), x.topk(k, dim=1).indices), a

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / ITERS * 1e3

    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            us[k].append(window(fn))
    out = {}
    for k, v in us.items():
        med = statistics.median(v)
        shape = k.rsplit("_rows_topk", 1)[0] if k.endswith("_rows_topk") else k.rsplit("_torch", 1)[0]
        out[k] = {"us_median": med, "us_min": min(v), "us_max": max(v), "matrix_GB_per_s": nbytes[shape] / med * 1e-3}
    for shape in nbytes:
        out[f"{shape}_torch_over_rows_topk"] = out[f"{shape}_torch"]["us_median"] / out[f"{shape}_rows_topk"]["us_median"]
    return out


def bench_fill(m):
    import torch
    from rmcl_amd import Predictor
    pr = Predictor(m)
    g = torch.Generator().manual_seed(1)
    cases = {}
    for B in (1, 64):
        ids = torch.randint(1000, 30522, (B, 40), generator=g)
        ids[:, 0], ids[:, -1] = 101, 102
        ids[:, [3, 9, 17, 24, 31]] = 103
        cases[f"B{B}_5masks"] = (ids, (torch.rand(B, 3, 384, 384, generator=g) * 2 - 1).to(m.engine.device))

    def window(name):
        ids, img = cases[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pr.fill_mask(img, text_ids=ids, mask_token_id=103)
        torch.cuda.synchronize()
        assert int((res["ids"] == 103).sum()) == 0 and all(len(f) == 5 for f in res["fills"])
        return (time.perf_counter() - t0) * 1e3

    for name in cases:
        window(name)
    ms = {name: [] for name in cases}
    for _ in range(LOOP_ROUNDS):
        for name in cases:
            ms[name].append(window(name))
    return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "rounds_per_call": 5} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.vilt.config import task_mlm_itm, _loss_names
    from rmcl_amd.vilt.modules import ViLTransformerSS
    torch.manual_seed(0)
    m = ViLTransformerSS(task_mlm_itm(per_gpu_batchsize=64, drop_rate=0.1, loss_names=_loss_names({"mlm": 1})), device="cuda:0", compute_dtype="bf16")
    rec = {"what": "Engine.rows_topk against torch (softmax / sigmoid + topk) on the stream, and Predictor.fill_mask end to end (12 layers, bf16)",
           "iters_per_window": ITERS, "rounds": ROUNDS, "single_run": True, "kernel_us": bench_kernels(m.engine), "fill_mask_ms": bench_fill(m)}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
