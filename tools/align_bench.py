"""Speed of the alignment path (needs the GPU): rmcl_ipot_plan_f32 against rmcl_ipot_f32 at the demo's 1000 iterations, and
``Predictor.align`` end to end.

Method: device events around WINDOW_LAUNCHES launches, 20 windows per arm, the two arms alternating window by window in one process, one
run; per arm the smallest, median and largest window (ms per launch).  Inputs: random unit features in 768 dimensions (costs near 1, the
`unit` family of tests/test_wpa_kernels_gpu.py), every slot valid but the three the demo's masks drop, beta 0.1.  The new kernel "wins" a
shape when its LARGEST window is below the old kernel's SMALLEST.  End to end: a 12-layer bf16 model on 384 x 384 images, wall clock
around align(...) with a device synchronisation, median of 20 calls after 3 warm-up calls.

Usage:  python tools/align_bench.py [--out profiles/align_bench.json]
"""
from __future__ import annotations

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
from rmcl_amd import Predictor  # noqa: E402
from rmcl_amd._lib import lib, check, P, F  # noqa: E402
from rmcl_amd.runtime import stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_moco  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402

DEV = "cuda:0"
WINDOWS, WINDOW_LAUNCHES, ITERS, BETA = 20, 4, 1000, 0.1


def inputs(B, Lt, Li, seed):
    g = torch.Generator().manual_seed(seed)
    xt = torch.nn.functional.normalize(torch.randn(B, Lt, 768, generator=g), dim=-1)
    xi = torch.nn.functional.normalize(torch.randn(B, Li, 768, generator=g), dim=-1)
    tv, iv = torch.ones(B, Lt, dtype=torch.int32), torch.ones(B, Li, dtype=torch.int32)
    tv[:, 0], tv[:, -1], iv[:, 0] = 0, 0, 0
    ld = (Li + 3) // 4 * 4
    cost = torch.zeros(B, Lt, ld)
    cost[:, :, :Li] = (1.0 - xt @ xi.transpose(1, 2)).masked_fill((tv[:, :, None] == 0) | (iv[:, None, :] == 0), 0.0)
    return cost.to(DEV), tv.to(DEV), iv.to(DEV)


def window(fn, cost, tv, iv, T):
    B, Lt, ld = cost.shape
    Li = iv.shape[1]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(WINDOW_LAUNCHES):
        check(fn(P(cost), P(tv), P(iv), P(T), B, Lt, Li, ld, F(BETA), ITERS, stream_ptr()), "ipot")
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / WINDOW_LAUNCHES


def bench_kernels():
    out = []
    for Li in (145, 241):
        for B in (1, 64):
            cost, tv, iv = inputs(B, 40, Li, seed=Li + B)
            T_old, T_new = torch.empty(B, Li, 40, device=DEV), torch.empty(B, Li, 40, device=DEV)
            arms = {"rmcl_ipot_f32": (lib.rmcl_ipot_f32, T_old, []), "rmcl_ipot_plan_f32": (lib.rmcl_ipot_plan_f32, T_new, [])}
            for fn, T, _ in arms.values():
                window(fn, cost, tv, iv, T)                                # warm-up
            for _ in range(WINDOWS):
                for fn, T, ms in arms.values():
                    ms.append(window(fn, cost, tv, iv, T))
            rec = {"Lt": 40, "Li": Li, "B": B, "iters": ITERS, "beta": BETA, "max_abs_difference_of_the_plans": float((T_old - T_new).abs().max())}
            for name, (_, _, ms) in arms.items():
                rec[name] = {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms)}
            rec["new_largest_below_old_smallest"] = rec["rmcl_ipot_plan_f32"]["max_ms"] < rec["rmcl_ipot_f32"]["min_ms"]
            rec["speedup_of_medians"] = rec["rmcl_ipot_f32"]["median_ms"] / rec["rmcl_ipot_plan_f32"]["median_ms"]
            print(json.dumps(rec))
            out.append(rec)
    return out


def bench_align():
    out = []
    cfg = task_moco(num_layers=12, num_negative=1024, per_gpu_batchsize=64, drop_rate=0.0, image_view=True)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype="bf16")
    pr = Predictor(m)
    g = torch.Generator().manual_seed(1)
    for B in (1, 64):
        ids = torch.randint(1000, 30522, (B, 40), generator=g)
        ids[:, 0], ids[:, -1] = 101, 102
        masks = torch.ones(B, 40, dtype=torch.int64)
        img = (torch.rand(B, 3, 384, 384, generator=g) * 2 - 1).to(DEV)
        ms = []
        for i in range(3 + WINDOWS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pr.align(img, text_ids=ids, text_masks=masks, token=5)
            torch.cuda.synchronize()
            if i >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"align_end_to_end": True, "B": B, "layers": 12, "dtype": "bf16", "iterations": 1000, "min_ms": min(ms),
               "median_ms": statistics.median(ms), "max_ms": max(ms)}
        print(json.dumps(rec))
        out.append(rec)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    args = ap.parse_args()
    res = {"method": f"device events, {WINDOWS} windows of {WINDOW_LAUNCHES} launches per arm, arms alternating in one process; ms per launch",
           "kernels": bench_kernels(), "align": bench_align()}
    res["new_kernel_wins_every_shape"] = all(r["new_largest_below_old_smallest"] for r in res["kernels"])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
