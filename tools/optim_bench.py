"""What the guarded optimizer step costs over the plain one, on the parameter arena of ViLT-B/32 (12 layers, rmcl_param_layout's total,
~112 M fp32 elements), with and without the bf16 shadow.

Per leg (one child process each, under its own time limit; a failed leg ends the run): after a warm-up of every kernel, ROUNDS rounds
that ALTERNATE four windows of ITERS calls each, timed with device events -
    plain          rmcl_adamw_f32
    guarded        rmcl_grad_stats_f32 + rmcl_adamw_guarded_f32   (what FusedAdamW.step() enqueues with the guard on)
    stats          rmcl_grad_stats_f32 alone
    guarded_adamw  rmcl_adamw_guarded_f32 alone (on the last decision)
and, in the same rounds, the other two update rules (rmcl_optim_step_f32), each as FusedAdam / FusedSGD enqueue them -
    adam_plain, sgd_plain        the plain form
    adam_guarded, sgd_guarded    rmcl_grad_stats_f32 + the guarded form
and reports the median and the spread of the per-call time over the rounds, the bytes each call must move (AdamW and Adam: 16 B read +
12 B written per element, SGD: 12 B + 8 B, each + 2 B with the shadow; statistics: 4 B read) and the rate that gives.
`added_over_plain` is the measured (guarded - plain) / plain; `bytes_estimate` is 4 / (28 or 30), what the statistics pass adds by byte
count.  `vs_adamw` holds, per new arm, its time over rmcl_adamw_f32's next to the ratio of the bytes.

  python tools/optim_bench.py --out profiles/optim_rules_bench.json        (profiles/guarded_step_bench.json: the first four arms, 10 rounds)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS, ROUNDS, WARMUP = 50, 20, 5
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

    adam_hyper = (F(1e-4), F(0.9), F(0.999), F(1e-8))
    sgd_hyper = (F(1e-4), F(0.9), F(0.0), F(0.0))

    def rule(code, vv, hp, with_ctl):                       # the arenas are shared between the arms: only the time is read
        def call():
            t[0] += 1
            if with_ctl:
                check(lib.rmcl_grad_stats_f32(P(g), I64(n), F(1.0), F(1.0), hp[1], hp[2], P(ws), P(ctl), s), "grad_stats")
            check(lib.rmcl_optim_step_f32(code, P(p), P(g), P(m), P(vv), P(lp), P(seg_end), P(mult), P(wd), nseg, *hp, t[0], F(1.0),
                                          P(ctl if with_ctl else None), I64(n), s), "optim_step")
        return call

    arms = {"plain": plain, "guarded": guarded, "stats": stats, "guarded_adamw": guarded_adamw,
            "adam_plain": rule(L.OPTIM_ADAM, v, adam_hyper, False), "adam_guarded": rule(L.OPTIM_ADAM, v, adam_hyper, True),
            "sgd_plain": rule(L.OPTIM_SGD, None, sgd_hyper, False), "sgd_guarded": rule(L.OPTIM_SGD, None, sgd_hyper, True)}
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
    sgd_bytes = n * (22 if shadow else 20)
    new_arms = (("adam_plain", adam_bytes), ("adam_guarded", adam_bytes + stat_bytes), ("sgd_plain", sgd_bytes), ("sgd_guarded", sgd_bytes + stat_bytes))
    for k, b in (("plain", adam_bytes), ("guarded", adam_bytes + stat_bytes), ("stats", stat_bytes), ("guarded_adamw", adam_bytes)) + new_arms:
        med = statistics.median(ms[k])
        out[k] = {"ms_median": med, "ms_min": min(ms[k]), "ms_max": max(ms[k]), "bytes": b, "TB_per_s": b / (med * 1e-3) / 1e12}
    out["added_over_plain"] = (out["guarded"]["ms_median"] - out["plain"]["ms_median"]) / out["plain"]["ms_median"]
    out["bytes_estimate"] = stat_bytes / adam_bytes
    out["vs_adamw"] = {k: {"time_ratio": out[k]["ms_median"] / out["plain" if k.endswith("plain") else "guarded"]["ms_median"],
                           "bytes_ratio": b / (adam_bytes if k.endswith("plain") else adam_bytes + stat_bytes)} for k, b in new_arms}
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
    rec = {"what": "rmcl_adamw_f32 against rmcl_grad_stats_f32 + rmcl_adamw_guarded_f32, and rmcl_optim_step_f32 (Adam, SGD) plain and "
                   "guarded beside them, ViLT-B/32 arena", "legs": legs}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
