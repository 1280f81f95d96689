#!/usr/bin/env python3
"""GPU: one hash per output of the MLM and the MPP head's C entry points, to compare two builds of the library bit for bit.

  RMCL_LIB=<library> python tools/pred_head_bits.py --out a.json        every case twice in this process: {case: {output: [hash, hash]}}
  python tools/pred_head_bits.py --compare ref.json new.json --out r.json    (no GPU) the verdict, as tools/encoder_bits.py gives it

The cases and the calls are the two kernel test modules' own (tests/test_mlm_gpu.py: _kernel_case / _run_kernels, tests/test_mpp_kernels_gpu.py:
_head_case / _run_head: compact, [weight transpose,] forward, backward with G and dxn, logits): the MLM module's parametrised set, MPP's
n in {1, 127, 128, 129, 300} x D in {256, 768}, both operand types, and the all-ignored batch of each head.  Outputs: idx, lab, count, lse,
rowloss, argmax, stats, G, dxn and the dense logits.  Both heads are bit-reproducible, so the verdict expects EVERY hash to equal the
reference library's; an output the reference does not reproduce against itself is listed by name and is a finding."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from encoder_bits import compare, digest  # noqa: E402

OUTPUTS = ("idx", "lab", "cnt", "lse", "rowloss", "argmax", "stats", "G", "dxn", "logits")
MLM_CASES = [(1, 30522, 768), (37, 30522, 768), (384, 30522, 768), (2560, 30522, 768), (37, 1000, 768), (384, 1000, 768), (1, 1000, 768),
             (1, 1000, 256), (37, 1000, 256)]
MPP_N = (1, 127, 128, 129, 300)


def cases():
    """[(label, callable -> result dict of device tensors)]"""
    from tests import test_mlm_gpu as A
    from tests import test_mpp_kernels_gpu as B
    out = []
    for dtype in ("f32", "bf16"):
        for n, V, D in MLM_CASES:
            def mlm(n=n, V=V, D=D, dtype=dtype):
                h, specs, arena, w, xn, labels, N = A._kernel_case(n, V, 1000 + n + V + (0 if D == 768 else D), D=D)
                return A._run_kernels(h, arena, xn, labels, N, dtype, gscale=0.5)
            out.append((f"mlm:n{n}:V{V}:D{D}:{dtype}", mlm))

        def mlm0(dtype=dtype):
            h, specs, arena, w, xn, labels, N = A._kernel_case(0, 1000, 3)
            return A._run_kernels(h, arena, xn, labels, N, dtype)
        out.append((f"mlm:all_ignored:{dtype}", mlm0))
        for D in (256, 768):
            for n in MPP_N + (0,):
                def mpp(n=n, D=D, dtype=dtype):
                    h, specs, arena, w, xn, labels, masked, Lt, N = B._head_case(n, D, 2000 + n + D if n else 7)
                    return B._run_head(h, arena, xn, labels, masked, Lt, N, dtype, gscale=0.5 if n else 1.0)
                out.append((f"mpp:{f'n{n}' if n else 'all_ignored'}:D{D}:{dtype}", mpp))
    return out


def measure(out):
    res = {}
    for label, go in cases():
        runs = [go(), go()]
        res[label] = {k: [digest(r[k].cpu()) for r in runs] for k in OUTPUTS if runs[0][k] is not None}
        print(label, json.dumps(res[label]), flush=True)
    with open(out, "w") as f:
        json.dump({"library": os.environ.get("RMCL_LIB", "(the tree's own)"), "hashes": res}, f, indent=1)
        f.write("\n")


def verdict(ref_path, new_path, out):
    rc = compare(ref_path, new_path, out)
    loose = json.load(open(out))["not_reproduced_by_the_reference"]
    if loose:
        print(f"FINDING: the reference library does not reproduce {loose} across its own two runs")
    return 1 if rc or loose else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare", nargs=2, metavar=("REF", "NEW"))
    a = ap.parse_args()
    sys.exit(verdict(*a.compare, a.out) if a.compare else measure(a.out))
