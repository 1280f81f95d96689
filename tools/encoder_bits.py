#!/usr/bin/env python3
"""GPU: one hash per output of the encoder passes, to compare two builds of the library bit for bit.

  RMCL_LIB=<library> python tools/encoder_bits.py --out a.json        every label twice in this process: {label: {output: [hash, hash]}}
  python tools/encoder_bits.py --compare ref.json new.json --out r.json    (no GPU) the verdict

The passes are those of tests/test_encoder_fp64_gpu.py - its run() with its contract (guard zones, NaN-filled buffers, inputs unchanged) and
its cases - under the same tune keys, plus two passes at the benchmark's shape (B 64, L 40, P 144, D 768, 12 layers, bf16): DATA with the
LayerNorm fold and the transposed weight shadows, FULL with a side stream set.  Outputs: xn, co, dpatches, dtext, G as the pass has them.

Verdict: every output the reference library reproduces across its own two runs must have the same hash under the other library (both runs).
Outputs the reference does not reproduce (fp32 atomics: the weight gradients of the non-grouped fp32 path, the embedding scatter) are listed
by name; the float64 tests bound them."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BENCH = dict(D=768, H=12, mlp=3072, layers=12, B=64, L=40, P=144, bf16=True)


def digest(t):
    import torch
    return hashlib.sha256(t.contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def passes():
    """[(label, callable -> result dict of CPU tensors)]"""
    import torch
    from tests import encoder_cases as T
    from tests import test_encoder_fp64_gpu as E
    from tests.gpu_util import L, lib
    T.SHAPES["bench"] = BENCH                      # (sorts behind the upper-case names: the other cases keep their seeds)
    get = T.get_case

    def G0(c):
        return torch.randn(c.total, generator=torch.Generator().manual_seed(77)) * 1e-3

    def run(name, mode, keys=None, dxn="full", **kw):
        def go():
            c = get(name)
            m = T.MODES[mode]
            if mode != "infer":
                kw["dxn"] = c.dxn[:, 0] if kw.get("cls_only") else (c.dxn if dxn == "full" else c.dxn_cls).reshape(-1, c.dims.D)
            if mode == "full":
                kw["G0"] = G0(c)
            with E.Keys(**(keys or {})):
                return E.run(c, m, **kw)
        return go

    def side_stream_full():
        s = torch.cuda.Stream()
        lib.rmcl_set_side_stream(C.c_void_p(s.cuda_stream))
        try:
            return run("bench", "full", lpT=True)()
        finally:
            torch.cuda.synchronize()
            lib.rmcl_set_side_stream(C.c_void_p(0))

    tail = dict(dxn="cls", tail=True, cls_only=2)
    out = [(f"A:{m}", run("A", m)) for m in ("infer", "data", "full")]
    out += [("D:full", run("D", "full")),
            ("F:data", run("A", "data", replaced=T.REPLACED_A)), ("F:full", run("A", "full", replaced=T.REPLACED_A)),
            ("G:cls_tail", run("A", "full", **tail)),
            ("H:dropout", run("A", "full", drop_p=0.25)),
            ("I:rank", lambda: {k: v for k, v in E.run_rank(get("I")).items() if k in ("xn", "co")}),
            ("K:infer:fold60", run("K", "infer", dict(k0=60), fold=True)), ("K:data:fold60", run("K", "data", dict(k0=60), fold=True, lpT=True)),
            ("K:data:tiled70", run("K", "data", dict(k0=70), fold=True, lpT=True, expect_tiled=True)),
            ("K:full:tiled70", run("K", "full", dict(k0=70), lpT=True, expect_tiled=True)),
            ("K2:infer:fold60", run("K2", "infer", dict(k0=60), fold=True)), ("K2:data:fold60", run("K2", "data", dict(k0=60), fold=True, lpT=True)),
            ("L4:full", run("L4", "full", lpT=True)), ("L3:full", run("L3", "full", lpT=True)),
            ("G:cls_tail:data", run("A", "data", **tail)), ("H:dropout:cls_tail", run("A", "full", drop_p=0.25, **tail)),
            ("L4:cls_tail:full", run("L4", "full", lpT=True, **tail)), ("J:cls_tail:data", run("J", "data", **tail)),
            ("bench:data:fold_lpT", run("bench", "data", fold=True, lpT=True)), ("bench:full:side_stream", side_stream_full)]
    return out


def measure(out):
    res = {}
    for label, go in passes():
        runs = [go(), go()]
        res[label] = {k: [digest(r[k]) for r in runs] for k in ("xn", "co", "dpatches", "dtext", "G") if k in runs[0]}
        print(label, json.dumps(res[label]), flush=True)
    with open(out, "w") as f:
        json.dump({"library": os.environ.get("RMCL_LIB", "(the tree's own)"), "hashes": res}, f, indent=1)
        f.write("\n")


def compare(ref_path, new_path, out):
    ref, new = (json.load(open(p))["hashes"] for p in (ref_path, new_path))
    assert set(ref) == set(new), sorted(set(ref) ^ set(new))
    same, differ, loose = [], [], []
    for label in ref:
        assert set(ref[label]) == set(new[label]), label
        for k, (a, b) in ref[label].items():
            name = f"{label}:{k}"
            if a != b:
                loose.append(name)
            elif new[label][k] == [a, a]:
                same.append(name)
            else:
                differ.append(name)
    verdict = {"condition": "every output the reference library reproduces across its own two runs has the same hash under the new library, in both runs",
               "met": not differ, "outputs": len(same) + len(differ) + len(loose), "identical": len(same), "different": differ,
               "not_reproduced_by_the_reference": loose}

    def row(label):                                # an identical output: its one hash; any other: the two runs of each library
        return {k: (a if f"{label}:{k}" in same else {"reference": [a, b], "new": new[label][k]}) for k, (a, b) in ref[label].items()}
    with open(out, "w") as f:                      # one line per label
        f.write("{" + ", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in verdict.items()) + ',\n "hashes": {\n')
        f.write(",\n".join(f"  {json.dumps(label)}: {json.dumps(row(label))}" for label in ref) + "}}\n")
    print(f"{len(same)} identical, {len(differ)} different {differ}, {len(loose)} the reference does not reproduce {loose}")
    return 0 if not differ else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare", nargs=2, metavar=("REF", "NEW"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare, a.out) if a.compare else measure(a.out))
