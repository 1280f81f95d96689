"""-m gpu: rmcl_rows_topk (csrc/topk.hip) through the C ABI against the float64 / integer statement of tests/topk_ref.py.

idx is exact and val is the input element bit for bit in every case; prob and lse lie within the allowance derived in tests/topk_ref.py
(checked on the CPU in tests/test_topk_ref_cpu.py); a second call gives the same bytes; a rejected call writes nothing.

Shapes.  C around the float4 group (1, 3, 4, 5), the wave (63 .. 65), the workgroup's first sweep of 256 threads (255 .. 257) and of 256
float4 groups (1023 .. 1025), the VQA head's 3129 and the vocabulary's 30522; R = 1, 2, 130; k = 1, 2, 5, 10, 32 wherever k <= C; pitches
C, C + 1 (every row at another alignment) and C + 7; the matrix begins 4 bytes into its allocation, so row 0 is never 16-byte aligned.
Guards.  The words in front of the matrix, behind it and in its pad columns hold 3e38: larger than every entry, so a read outside
[row, row + C) would win the first place of that row (a NaN guard would be invisible to this kernel - NaN is never selected and adds
nothing to the log-sum-exp - and is therefore used on the output side, where bytes are compared).  idx / val / prob / lse lie between
guard words that must keep their bits.
Rows (cycled over the rows of a matrix): a random permutation of an arithmetic progression (no near tie by construction); exact ties
across the float4 (3 | 4), wave (63 | 64), workgroup (255 | 256), float4-sweep (1023 | 1024) boundaries and in the last column; an
all-equal row; the maximum in the first / in the last column; ascending; descending; -inf columns; a row with fewer than k selectable
columns because of NaNs; values at +-80.
The largest |error| / allowance goes to the file named by RMCL_PREDICT_PARITY_OUT when set (profiles/predict_parity.json is such a dump)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib  # noqa: E402
from tests import topk_ref as T  # noqa: E402
from tests.gpu_util import DEV, stream  # noqa: E402

COLS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3129, 30522)
ROWS = (1, 2, 130)
KS = (1, 2, 5, 10, 32)
MODES = {"raw": L.TOPK_RAW, "softmax": L.TOPK_SOFTMAX, "sigmoid": L.TOPK_SIGMOID}
SENTINEL = 3.0e38
GUARD = 16                                            # guard words on each side of every buffer (a multiple of 4: the offset below is the 4 bytes)
I_GUARD, F_GUARD = 0x7FC0DEAD, float("nan")
WORST = {"lse": [0.0, None], "prob_softmax": [0.0, None], "prob_sigmoid": [0.0, None]}
N_KINDS = 10


def make_row(kind, Cn, g):
    """one row [C] float32 of the kind `kind` (module docstring)"""
    f = np.float32
    prog = (np.arange(Cn, dtype=np.float64) / 256.0 - Cn / 512.0).astype(f)          # exact in fp32 up to C = 30522
    if kind == 0:
        return g.permutation(prog)
    if kind == 1:
        row = g.permutation(prog)
        top = f(row.max() + 1.0)
        for c in (3, 4, 63, 64, 255, 256, 1023, 1024, 1027, Cn - 1):                  # one tied maximum on both sides of every boundary
            if c < Cn:
                row[c] = top
        if Cn > 8:
            row[[1, Cn - 2]] = f(row.min() - 1.0)                                     # and a tied minimum
        return row
    if kind == 2:
        return np.full(Cn, 0.75, dtype=f)
    if kind == 3 or kind == 4:
        row = g.permutation(prog)
        row[0 if kind == 3 else Cn - 1] = f(row.max() + 0.5)
        return row
    if kind == 5:
        return prog.copy()
    if kind == 6:
        return prog[::-1].copy()
    if kind == 7:
        row = g.permutation(prog)
        row[::3] = -np.inf
        return row
    if kind == 8:                                                                      # at most 3 selectable columns, one of them -inf
        row = np.full(Cn, np.nan, dtype=f)
        keep = g.permutation(Cn)[:3]
        row[keep] = np.array([1.5, -np.inf, -2.0], dtype=f)[: keep.size]
        return row
    row = np.where(g.random(Cn) < 0.5, 80.0, -80.0).astype(f)                          # kind 9: +-80
    row[g.integers(0, Cn)] = 79.0
    return row


def make_matrix(R, Cn):
    g = np.random.default_rng(1000 * Cn + R)
    first = {1: 0, 2: 1}.get(R, 0)                                                     # R = 1: the permutation; R = 2: ties, then the all-equal row
    x = np.stack([make_row((first + r) % N_KINDS, Cn, g) for r in range(R)])
    if R == 2:
        x[1] = make_row(8, Cn, g)                                                      # ... and the NaN row
    return x


class Reference:
    """the float64 model of one matrix, computed once: the full selection order of every row, lse and its allowance"""

    def __init__(self, x):
        self.x = x
        self.order = [T.order(r) for r in x]
        self.lse = np.array([T.lse_row(r) for r in x])
        self.lse_allow = np.array([T.lse_allowance(r) for r in x])

    def topk(self, k, mode):
        R = self.x.shape[0]
        idx = np.full((R, k), -1, dtype=np.int32)
        val = np.full((R, k), -np.inf, dtype=np.float32)
        prob = np.zeros((R, k))
        for r in range(R):
            o = self.order[r][:k]
            idx[r, : o.size] = o
            val[r, : o.size] = self.x[r, o]
            v = self.x[r, o].astype(np.float64)
            with np.errstate(over="ignore", invalid="ignore"):
                if mode == "softmax":
                    prob[r, : o.size] = np.where(np.isneginf(v), 0.0, np.exp(v - self.lse[r]))
                elif mode == "sigmoid":
                    prob[r, : o.size] = 1.0 / (1.0 + np.exp(-v))
        return idx, val, prob


def guarded(n, dtype, fill):
    t = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
    t.fill_(fill)
    return t


def guards_intact(t, n, fill):
    want = torch.full((GUARD,), fill, dtype=t.dtype)
    a, b = t[:GUARD].cpu(), t[GUARD + n:].cpu()
    if t.dtype == torch.float32:
        a, b, want = a.view(torch.int32), b.view(torch.int32), want.view(torch.int32)
    return torch.equal(a, want) and torch.equal(b, want)


def place(x, ld):
    """x [R, C] at pitch ld, 4 bytes into an allocation whose every other word is the sentinel: (device buffer, element offset of x[0, 0])"""
    R, Cn = x.shape
    off = GUARD + 1
    host = np.full(off + R * ld + GUARD, SENTINEL, dtype=np.float32)
    view = host[off: off + R * ld].reshape(R, ld)
    view[:, :Cn] = x
    return torch.from_numpy(host).to(DEV), off


def run(buf, off, ld, R, Cn, k, mode, want_lse=True):
    idx, val = guarded(R * k, torch.int32, I_GUARD), guarded(R * k, torch.float32, F_GUARD)
    prob, lse = guarded(R * k, torch.float32, F_GUARD), guarded(R, torch.float32, F_GUARD)
    x_ptr = C.c_void_p(buf.data_ptr() + 4 * off)
    p = lambda t: C.c_void_p(t.data_ptr() + 4 * GUARD)
    rc = lib.rmcl_rows_topk(x_ptr, C.c_int64(ld), R, Cn, k, MODES[mode], p(idx), p(val), p(prob) if mode != "raw" else None,
                            p(lse) if (want_lse and mode == "softmax") else None, stream())
    torch.cuda.synchronize()
    return rc, idx, val, prob, lse


def note(key, ratio, where):
    if ratio > WORST[key][0]:
        WORST[key] = [float(ratio), where]


@pytest.fixture(scope="module", autouse=True)
def parity_dump():
    yield
    out = os.environ.get("RMCL_PREDICT_PARITY_OUT")
    if out:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec["rows_topk"] = {"what": "largest |kernel - float64 model| / allowance (tests/topk_ref.py) over every case of tests/test_topk_kernels_gpu.py",
                            **{k: {"ratio": v[0], "at": v[1]} for k, v in WORST.items()}}
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("Cn", COLS)
def test_rows_topk_matches_the_model(Cn):
    for R in ROWS:
        x = make_matrix(R, Cn)
        ref = Reference(x)
        for ld in (Cn, Cn + 1, Cn + 7):
            buf, off = place(x, ld)
            before = buf.clone()
            for k in (k for k in KS if k <= Cn):
                for mode in MODES:
                    where = f"C={Cn} R={R} ld={ld} k={k} {mode}"
                    rc, idx, val, prob, lse = run(buf, off, ld, R, Cn, k, mode)
                    assert rc == 0, (where, lib.rmcl_last_error())
                    n = R * k
                    assert guards_intact(idx, n, I_GUARD) and guards_intact(val, n, F_GUARD) and guards_intact(prob, n, F_GUARD), where
                    assert guards_intact(lse, R, F_GUARD), where
                    gi = idx[GUARD: GUARD + n].cpu().numpy().reshape(R, k)
                    gv = val[GUARD: GUARD + n].cpu().numpy().reshape(R, k)
                    wi, wv, wp = ref.topk(k, mode)
                    assert np.array_equal(gi, wi), (where, np.argwhere(gi != wi)[:4])
                    assert np.array_equal(gv.view(np.int32), wv.view(np.int32)), where          # the input element, bit for bit
                    gp = prob[GUARD: GUARD + n].cpu().numpy().reshape(R, k)
                    gl = lse[GUARD: GUARD + R].cpu().numpy()
                    if mode == "raw":
                        assert np.isnan(gp).all() and np.isnan(gl).all(), where                # prob / lse untouched
                    else:
                        assert not np.isnan(gp).any(), where
                        for r in range(R):
                            allow = T.prob_allowance(x[r], wv[r], wp[r], mode)
                            ratio = np.abs(gp[r].astype(np.float64) - wp[r]) / allow
                            assert ratio.max() <= 1.0, (where, r, gp[r], wp[r], allow)
                            note(f"prob_{mode}", ratio.max(), f"{where} row {r}")
                            assert np.all(gp[r][wi[r] < 0] == 0.0), where                      # unfilled slots: exactly 0
                    if mode == "softmax":
                        none = np.isneginf(ref.lse)
                        assert np.all(np.isneginf(gl[none])), where
                        if (~none).any():
                            ratio = np.abs(gl[~none].astype(np.float64) - ref.lse[~none]) / ref.lse_allow[~none]
                            assert ratio.max() <= 1.0, (where, gl, ref.lse, ref.lse_allow)
                            note("lse", ratio.max(), where)
                    else:
                        assert np.isnan(gl).all(), where                                       # lse is written in softmax mode only
                    rc2, idx2, val2, prob2, lse2 = run(buf, off, ld, R, Cn, k, mode)
                    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
                    assert rc2 == 0 and same(idx, idx2) and same(val, val2) and same(prob, prob2) and same(lse, lse2), where
            assert torch.equal(buf.view(torch.int32), before.view(torch.int32))                 # the input is read only


def test_prob_and_lse_pointers_are_optional():
    x = make_matrix(130, 257)
    ref = Reference(x)
    buf, off = place(x, 258)
    rc, idx, val, prob, lse = run(buf, off, 258, 130, 257, 5, "softmax", want_lse=False)
    assert rc == 0 and torch.isnan(lse).all()
    wi, wv, _ = ref.topk(5, "softmax")
    assert np.array_equal(idx[GUARD:-GUARD].cpu().numpy().reshape(130, 5), wi)
    idx2, val2 = guarded(650, torch.int32, I_GUARD), guarded(650, torch.float32, F_GUARD)
    p = lambda t: C.c_void_p(t.data_ptr() + 4 * GUARD)
    for mode in MODES.values():                                                               # prob NULL in every mode
        assert lib.rmcl_rows_topk(C.c_void_p(buf.data_ptr() + 4 * off), C.c_int64(258), 130, 257, 5, mode, p(idx2), p(val2), None, None, stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(idx2[GUARD:-GUARD].cpu().numpy().reshape(130, 5), wi) and guards_intact(idx2, 650, I_GUARD)
        assert np.array_equal(val2[GUARD:-GUARD].cpu().numpy().reshape(130, 5).view(np.int32), wv.view(np.int32))


def test_rejected_calls_return_an_error_and_write_nothing():
    x = make_matrix(2, 64)
    buf, off = place(x, 64)
    bad = [dict(k=0), dict(k=33), dict(Cn=4, k=5), dict(Cn=0, k=1), dict(ld=63), dict(mode=3), dict(R=-1), dict(null="x"), dict(null="idx"), dict(null="val"),
           dict(shift=2)]
    for kw in bad:
        idx, val = guarded(64, torch.int32, I_GUARD), guarded(64, torch.float32, F_GUARD)
        prob, lse = guarded(64, torch.float32, F_GUARD), guarded(2, torch.float32, F_GUARD)
        p = lambda t: C.c_void_p(t.data_ptr() + 4 * GUARD)
        a = dict(R=2, Cn=64, k=5, ld=64, mode=L.TOPK_SOFTMAX, null=None, shift=0)
        a.update(kw)
        xp = None if a["null"] == "x" else C.c_void_p(buf.data_ptr() + 4 * off + a["shift"])
        rc = lib.rmcl_rows_topk(xp, C.c_int64(a["ld"]), a["R"], a["Cn"], a["k"], a["mode"], None if a["null"] == "idx" else p(idx),
                                None if a["null"] == "val" else p(val), p(prob), p(lse), stream())
        torch.cuda.synchronize()
        assert rc == -1 and b"rows_topk" in lib.rmcl_last_error(), kw
        assert bool((idx == I_GUARD).all()) and all(bool(torch.isnan(t).all()) for t in (val, prob, lse)), kw
    idx = guarded(8, torch.int32, I_GUARD)
    assert lib.rmcl_rows_topk(C.c_void_p(buf.data_ptr() + 4 * off), C.c_int64(64), 0, 64, 4, L.TOPK_RAW, C.c_void_p(idx.data_ptr()),
                              C.c_void_p(idx.data_ptr()), None, None, stream()) == 0           # R = 0: nothing to do
    torch.cuda.synchronize()
    assert bool((idx == I_GUARD).all())
