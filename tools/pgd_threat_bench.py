#!/usr/bin/env python
"""Stream time of the PGD threat-model kernels (csrc/pgd_ball.hip) next to rmcl_pgd_step_fused, and one RobustEval.attack end to end.

Kernel arms, at the training step's own shape (B = 64, per_sample = 144 * 3072; bf16 gradient + bf16 operand, and the fp32 twin): every
threat model's step, the random starts, keep_worst and the fused reference step alternate in ONE process; per arm the median of 20 timed
calls (hip events around one call) after 5 warm-up rounds.  Bytes per call are computed from the shapes (the pass structure is stated in
csrc/pgd_ball.hip); bytes / median time gives the rate.

End to end: RobustEval.attack on a 12-layer bf16 VQA model, batch 128, K = 10, restarts 1 and 3; the share of the three new kernels is
their summed stream time at that batch (measured the same way) over the wall time of the call.

    python tools/pgd_threat_bench.py [--out profiles/pgd_threat_bench.json] [--skip-e2e]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P, I64, F  # noqa: E402

DEV = "cuda:0"
PER = 144 * 3072
BOX = (-1.0, 1.0)


def stream():
    return L.C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tdt(dt):
    return torch.float32 if dt == L.F32 else torch.bfloat16


def arms(B, dt, odt):
    """name -> (callable, bytes moved per call)"""
    g = (torch.randn(B, PER, device=DEV) * 1e-3).to(tdt(dt))
    delta = torch.zeros(B, PER, device=DEV)
    base = torch.rand(B, PER, device=DEV) * 2 - 1
    out = torch.empty(B, PER, dtype=tdt(odt), device=DEV)
    best_d, best_o = torch.empty_like(delta), torch.empty_like(out)
    amax = torch.empty(64 * B, dtype=torch.int32, device=DEV)
    scr = torch.empty(int(lib.rmcl_pgd_ball_scratch_bytes(B)), dtype=torch.uint8, device=DEV)
    valid = torch.full((B,), PER, dtype=torch.int32, device=DEV)
    score = torch.rand(B, 2, device=DEV)
    best_s = torch.zeros(B, device=DEV)
    best_r = torch.zeros(B, dtype=torch.int32, device=DEV)
    n = B * PER
    G, O = g.element_size(), out.element_size()
    step_bytes = n * (G + 4 + 4 + 4 + O)                       # the step pass: g, delta in, base, delta out, operand

    def step(direction, ball, lr, eps, box, v):
        lo, hi = box if box else (0.0, 0.0)
        return lambda: check(lib.rmcl_pgd_step_ball(P(g), dt, P(delta), P(scr), P(v), B, I64(PER), F(lr), F(eps), direction, ball, F(lo), F(hi), P(base),
                                                    P(out), odt, 0, stream()), "pgd_step_ball")

    def start(ball, eps):
        return lambda: check(lib.rmcl_pgd_random_start(P(delta), P(scr), None, B, I64(PER), 0, 17, F(eps), ball, F(-1.0), F(1.0), P(base), P(out), odt,
                                                       stream()), "pgd_random_start")

    return {
        "fused_reference_step": (lambda: check(lib.rmcl_pgd_step_fused(P(g), dt, P(delta), P(amax), B, I64(PER), F(0.01), F(0.005), P(base), P(out), odt, 0,
                                                                       stream()), "pgd_step_fused"), n * G + step_bytes),
        "normalised_linf": (step(L.PGD_DIR_NORMALISED, L.PGD_BALL_LINF, 0.01, 0.005, None, None), n * G + step_bytes),
        "normalised_linf_box_valid": (step(L.PGD_DIR_NORMALISED, L.PGD_BALL_LINF, 0.01, 0.005, BOX, valid), n * G + step_bytes + 2 * 4 * B),
        "sign_linf_box": (step(L.PGD_DIR_SIGN, L.PGD_BALL_LINF, 0.002, 0.005, BOX, None), step_bytes),
        "l2_l2_box": (step(L.PGD_DIR_L2, L.PGD_BALL_L2, 0.5, 1.0, BOX, None), n * G + n * (G + 4) + step_bytes),
        "random_start_linf": (start(L.PGD_BALL_LINF, 0.005), n * (4 + 4 + O)),
        "random_start_l2": (start(L.PGD_BALL_L2, 1.0), n * (4 + 4 + O)),
        "keep_worst_all_take": (lambda: check(lib.rmcl_pgd_keep_worst(P(score[:, 0]), I64(2), P(best_s), P(best_r), 0, B, 1, P(delta), P(best_d), P(out),
                                                                      P(best_o), odt, I64(PER), stream()), "pgd_keep_worst"), n * 2 * (4 + O)),
    }


def time_arms(table, rounds=20, warm=5):
    times = {k: [] for k in table}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(warm + rounds):
        for name, (fn, _) in table.items():                   # the arms alternate
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {}
    for name, (_, nbytes) in table.items():
        med = statistics.median(times[name])
        res[name] = {"median_us": round(med, 2), "min_us": round(min(times[name]), 2), "max_us": round(max(times[name]), 2), "bytes": int(nbytes),
                     "GB_per_s": round(nbytes / med / 1e3, 1)}
    return res


def end_to_end(kernels128):
    from rmcl_amd import RobustEval
    from rmcl_amd.vilt.config import task_finetune_vqa
    from rmcl_amd.vilt.modules import ViLTransformerSS
    B, K = 128, 10
    torch.manual_seed(0)
    m = ViLTransformerSS(task_finetune_vqa(num_layers=12, per_gpu_batchsize=B, drop_rate=0.0), device=DEV, compute_dtype="bf16")
    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30522, (B, 40), generator=gen)
    ids[:, 0], ids[:, -1] = 101, 102
    batch = {"text_ids": ids.to(DEV), "text_masks": torch.ones(B, 40, dtype=torch.int64, device=DEV),
             "image": [(torch.rand(B, 3, 384, 384, generator=gen) * 2 - 1).to(DEV)],
             "vqa_labels": [[int(i) % 3129] for i in range(B)], "vqa_scores": [[1.0] for _ in range(B)]}
    re = RobustEval(m)
    out = {}
    for restarts in (1, 3):
        ms = []
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            re.attack(batch, 4 / 255 * 2, steps=K, restarts=restarts, seed=rep)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        kern_us = restarts * (K * kernels128["sign_linf_box"]["median_us"] + kernels128["random_start_linf"]["median_us"] +
                              kernels128["keep_worst_all_take"]["median_us"])
        best = min(ms[1:])
        out[f"restarts_{restarts}"] = {"ms_runs": [round(v, 1) for v in ms], "ms": round(best, 1), "new_kernels_ms": round(kern_us / 1e3, 2),
                                       "new_kernels_share": round(kern_us / 1e3 / best, 4)}
    return {"B": B, "layers": 12, "dtype": "bf16", "K": K, "eps": "4/255 of [0, 1] = 8/255 of [-1, 1]", "first run of each is a warm-up": True, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    res = {"shape": {"B": 64, "per_sample": PER}, "rounds": 20, "warmup": 5, "kernels": {}}
    for tag, dt, odt in (("bf16_grad_bf16_operand", L.BF16, L.BF16), ("f32_grad_f32_operand", L.F32, L.F32)):
        res["kernels"][tag] = time_arms(arms(64, dt, odt))
    if not a.skip_e2e:
        k128 = time_arms(arms(128, L.BF16, L.BF16), rounds=10, warm=3)
        res["kernels_B128_bf16"] = {k: k128[k] for k in ("sign_linf_box", "random_start_linf", "keep_worst_all_take")}
        res["robust_eval_attack_vqa"] = end_to_end(k128)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
