#!/usr/bin/env python3
"""GPU: SHA-256 digests of what the GEMM epilogues write, for comparing two builds of the library bit for bit.

  RMCL_LIB=<library> python tools/gemm_epilogue_bits.py --out a.json        one library (default: this tree's build)
  python tools/gemm_epilogue_bits.py --merge a.json b.json --out profiles/gemm_epilogue_bits.json
                                                                             both digests per case; exit status 1 unless all are equal

Cases (a case's digest runs over its output buffers in a fixed order; "buffers" says how many):
  skinny/...   the five launches of tests/test_gemm_skinny_stream_gpu.py, every M and both weight layouts of that file, per (N, K) and
               epilogue, under rmcl_tune_set key 6 = 0 (row-split kernel), 1 (k-split kernel) and -1 (streaming form);
  encoder/...  the Case of tests/test_encoder_skinny_stream_gpu.py at dropout 0 and 0.1, key 6 = 1 and -1: the buffers that test compares
               bit for bit (x_final, stash, q, cls_feats, dcls, dpatches, dtext and the gradient pieces one workgroup owns);
  fast/, big/  the 128x128 and the 256x256 bf16 kernel (key 0 = 2 and 30; the route is asserted), bf16 in, bf16 and fp32 out: bias + GELU +
               stash, bias + residual, GELU' of a stash, accumulate (fp32 out), M in (1, 130, 257), N = 256, K in (64, 256), layouts NT and
               NN, and TN at M = 256."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def merge(a, b, out):
    A, B = json.load(open(a)), json.load(open(b))
    keys = sorted(set(A["cases"]) | set(B["cases"]))
    cases, bad = {}, []
    for k in keys:
        x, y = A["cases"].get(k), B["cases"].get(k)
        eq = x is not None and x == y
        cases[k] = {"buffers": (x or y)["buffers"], "before": x and x["sha256"], "after": y and y["sha256"], "equal": eq}
        if not eq:
            bad.append(k)
    res = {"before": A["library"], "after": B["library"], "device": B["device"], "cases": len(cases), "all_equal": not bad, "unequal": bad, "digests": cases}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"{len(cases)} cases, {len(bad)} unequal")
    return 1 if bad else 0


def run(out):
    import torch
    import tests.test_gemm_skinny_stream_gpu as S
    import tests.test_encoder_skinny_stream_gpu as E
    from tests.gpu_util import DEV, L, lib, check, gemm

    cases = {}

    def put(name, tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        assert name not in cases, name
        cases[name] = {"buffers": len(tensors), "sha256": h.hexdigest()}

    # 1. skinny fp32 family
    for N, K in S.NKS:
        Xall, W, Wn, bias, res_all, u_all, base_all, _ = S.operands(N, K)
        for form in (0, 1, -1):
            bufs = {}
            for M in S.MS:
                X, res, u = Xall[:M].contiguous(), res_all[:M].contiguous(), u_all[:M].contiguous()
                for b_kc, W_arg in ((1, W), (0, Wn)):
                    with S.Form(form):
                        got = S.epilogues(M, N, W_arg, b_kc, X, bias, res, u, base_all)
                    for name, outs in got.items():
                        bufs.setdefault(name, []).extend(outs)
            for name, ts in bufs.items():
                put(f"skinny/form{form}/N{N}_K{K}/{name}", ts)

    # 2. the cls-only tail and the heads, with and without dropout
    for B in (4, 3):
        case = E.Case(B)
        for p, seed in ((0.0, 0), (0.1, E.DROP_SEED)):
            for form in (1, -1):
                check(lib.rmcl_tune_set(6, form), "tune_set")
                try:
                    r = case.run(p, seed)
                finally:
                    check(lib.rmcl_tune_set(6, -1), "tune_set")
                ts = [r[k] for k in ("x_final", "stash", "q", "cls_feats", "dcls", "dpatches", "dtext")] + [r["G"][o:o + n] for o, n in case.owned()]
                put(f"encoder/form{form}/B{B}_p{p}", ts)

    # 3. the two bf16 kernels with the 4-column epilogue
    EPI_BIAS, EPI_GELU, EPI_SAVE_PREACT, EPI_RESIDUAL, EPI_DGELU, EPI_ACCUM = 1, 2, 4, 8, 16, 64
    rnd = S.rnd
    N = 256
    for fam, cfg, route in (("fast", 2, 0), ("big", 30, 5)):
        check(lib.rmcl_tune_set(0, cfg), "tune_set")
        try:
            for lay, a_kc, b_kc, Ms in (("NT", 1, 1, (1, 130, 257)), ("NN", 1, 0, (1, 130, 257)), ("TN", 0, 0, (256,))):
                for K in (64, 256):
                    for M in Ms:
                        A = rnd(*((M, K) if a_kc else (K, M)), seed=31).bfloat16()
                        Bm = rnd(*((N, K) if b_kc else (K, N)), seed=32, scale=0.05).bfloat16()
                        bias, res, base = rnd(N, seed=33), rnd(M, N, seed=34), rnd(M, N, seed=35)
                        stash = rnd(M, N, seed=36).bfloat16()
                        for dt_out, oname in ((L.BF16, "bf16"), (L.F32, "f32")):
                            g = lambda **kw: gemm(A, Bm, M, N, K, a_kc, b_kc, L.BF16, dt_out, exact=0, **kw)
                            launches = {"bias_gelu_stash": (EPI_BIAS | EPI_GELU | EPI_SAVE_PREACT, dict(bias=bias, want_c2=True)),
                                        "bias_residual": (EPI_BIAS | EPI_RESIDUAL, dict(bias=bias, aux=res, ld_aux=N)),
                                        "dgelu_of_stash": (EPI_DGELU, dict(aux=stash, ld_aux=N))}
                            if dt_out == L.F32:
                                launches["accum"] = (EPI_ACCUM, dict(C_init=base))
                            for name, (epi, kw) in launches.items():
                                got = lib.rmcl_gemm_route(M, N, K, epi, dt_out, a_kc, b_kc)
                                assert got == route, (fam, lay, M, K, name, got)
                                o = g(epi=epi, **kw)
                                put(f"{fam}/{lay}/M{M}_K{K}/{oname}/{name}", list(o) if isinstance(o, tuple) else [o])
        finally:
            check(lib.rmcl_tune_set(0, -1), "tune_set")

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {"library": os.path.relpath(os.environ["RMCL_LIB"], root) if os.environ.get("RMCL_LIB") else "this tree", "device": torch.cuda.get_device_name(0), "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"{len(cases)} cases written to {out}")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs=2, metavar=("BEFORE", "AFTER"))
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.exit(merge(*a.merge, a.out) if a.merge else run(a.out))
