"""What the guarded optimizer step costs over the plain one, on the parameter arena of ViLT-B/32 (12 layers, rmcl_param_layout's total,
~112 M fp32 elements), with and without the bf16 shadow.

Per leg (one child process each, under its own time limit; a failed leg ends the run): after a warm-up of every kernel, ROUNDS rounds
that ALTERNATE four windows of ITERS calls each, timed with device events -
    plain          rmcl_adamw_f32
    guarded        rmcl_grad_stats_f32 + rmcl_adamw_guarded_f32   (what FusedAdamW.step() enqueues with the guard on)
    stats          rmcl_grad_stats_f32 alone
    guarded_adamw  rmcl_adamw_guarded_f32 alone (on the last decision)
and reports the median and the spread of the per-call time over the rounds, the bytes each call must move (AdamW: 16 B read + 12 B
written per element, + 2 B with the shadow; statistics: 4 B read) and the rate that gives.  `added_over_plain` is the measured
(guarded - plain) / plain; `bytes_estimate` is 4 / (28 or 30), what the statistics pass adds by byte count.

  python tools/optim_bench.py --out profiles/guarded_step_bench.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS, ROUNDS, WARMUP = 50, 10, 5
LEG_TIMEOUT = 240


def leg(shadow: bool) -> dict:
    import torch
    import rmcl_pkg  # noqa: F401
    from rmcl_amd import _lib as L
    from rmcl_amd._lib import lib, check, P, I64, F
    dev = "cuda:0"
    d = L.Dims(B=64, L=40, P=144, D=768, H=12, layers=12, mlp=3072, patch_k=3072, proj=128, vocab=30522, dtype=1, exact=0)
    lay = L.Layout()
    lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    n = int(lay.total)
    nseg = 192                                              # about the tensor count of the arena; ends on 64-element boundaries
    ends = [min(n, ((n // nseg) * (i + 1)) // 64 * 64) for i in range(nseg - 1)] + [n]
    torch.manual_seed(0)
    p, g = torch.randn(n, device=dev) * 0.02, torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lp = torch.zeros(n, dtype=torch.bfloat16, device=dev) if shadow else None
    seg_end = torch.tensor(ends, dtype=torch.int64, device=dev)
    mult = torch.ones(nseg, device=dev)
    wd = torch.tensor([0.01 if i % 2 == 0 else 0.0 for i in range(nseg)], device=dev)
    ctl = torch.zeros(C.sizeof(L.StepCtl), dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(lib.rmcl_grad_stats_ws_bytes(I64(n))), dtype=torch.uint8, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hyper = (F(1e-4), F(0.9), F(0.98), F(1e-8))
    t = [0]

    def plain():
        t[0] += 1
        check(lib.rmcl_adamw_f32(P(p), P(g), P(m), P(v), P(lp), P(seg_end), P(mult), P(wd), nseg, *hyper, t[0], F(1.0), I64(n), s), "adamw")

    def stats():
        check(lib.rmcl_grad_stats_f32(P(g), I64(n), F(1.0), F(1.0), F(0.9), F(0.98), P(ws), P(ctl), s), "grad_stats")

    def guarded():
        stats()
        check(lib.rmcl_adamw_guarded_f32(P(p), P(g), P(m), P(v), P(lp), P(seg_end), P(mult), P(wd), nseg, *hyper, F(1.0), P(ctl), I64(n), s),
              "adamw_guarded")

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / ITERS

    def guarded_adamw():                                    # the AdamW half alone, on the decision the last statistics pass left
        check(lib.rmcl_adamw_guarded_f32(P(p), P(g), P(m), P(v), P(lp), P(seg_end), P(mult), P(wd), nseg, *hyper, F(1.0), P(ctl), I64(n), s),
              "adamw_guarded")

    arms = {"plain": plain, "guarded": guarded, "stats": stats, "guarded_adamw": guarded_adamw}
    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            ms[k].append(window(fn))
    c = L.StepCtl.from_tensor(ctl)
    assert c.skip == 0 and c.nonfinite == 0 and bool(torch.isfinite(p).all())
    adam_bytes, stat_bytes = n * (30 if shadow else 28), n * 4
    out = {"shadow": shadow, "elements": n, "segments": nseg, "iters_per_window": ITERS, "rounds": ROUNDS}
    for k, b in (("plain", adam_bytes), ("guarded", adam_bytes + stat_bytes), ("stats", stat_bytes), ("guarded_adamw", adam_bytes)):
        med = statistics.median(ms[k])
        out[k] = {"ms_median": med, "ms_min": min(ms[k]), "ms_max": max(ms[k]), "bytes": b, "TB_per_s": b / (med * 1e-3) / 1e12}
    out["added_over_plain"] = (out["guarded"]["ms_median"] - out["plain"]["ms_median"]) / out["plain"]["ms_median"]
    out["bytes_estimate"] = stat_bytes / adam_bytes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=["shadow", "noshadow"], default=None)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg == "shadow")))
        return 0
    legs = []
    for name in ("shadow", "noshadow"):                    # a fresh process per leg, each under its own time limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=LEG_TIMEOUT)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            return r.returncode
        legs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    rec = {"what": "rmcl_adamw_f32 against rmcl_grad_stats_f32 + rmcl_adamw_guarded_f32, ViLT-B/32 arena", "legs": legs}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
