"""CPU: the float64 statement of rmcl_rows_topk (tests/topk_ref.py) against torch.topk / torch.logsumexp; the rounding model behind the
prob / lse allowance, exercised on the kernel's own summation order in numpy float32; the compiler's assembly of csrc/topk.hip (every
launched instantiation present, no scratch, no float atomics, no compare-and-swap loop); and the argument checks of the entry point,
which precede the launch and therefore need no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import topk_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc", "topk.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]
KERNELS = ("rows_topk_kernelILb0EE", "rows_topk_kernelILb1EE")          # without / with the log-sum-exp (RAW and SIGMOID / SOFTMAX)


def _rows(seed, R, Cn):
    g = np.random.default_rng(seed)
    return np.stack([g.permutation(Cn).astype(np.float32) * 0.25 - 3.0 for _ in range(R)])      # distinct values per row


@pytest.mark.parametrize("Cn,k", [(1, 1), (5, 5), (65, 10), (1025, 32)])
def test_model_agrees_with_torch_on_distinct_values(Cn, k):
    x = _rows(Cn, 3, Cn)
    idx, val, prob, lse = T.rows_topk(x, k, "softmax")
    tv, ti = torch.from_numpy(x).topk(k, dim=1)
    assert np.array_equal(idx, ti.numpy().astype(np.int32)) and np.array_equal(val, tv.numpy())
    x64 = torch.from_numpy(x).double()
    np.testing.assert_allclose(lse, torch.logsumexp(x64, dim=1).numpy(), rtol=1e-13)
    np.testing.assert_allclose(prob, torch.softmax(x64, dim=1).gather(1, ti).numpy(), rtol=1e-12)
    _, _, ps, _ = T.rows_topk(x, k, "sigmoid")
    np.testing.assert_allclose(ps, torch.sigmoid(x64).gather(1, ti).numpy(), rtol=1e-12)
    assert T.rows_topk(x, k, "raw")[2] is None


def test_model_ties_values_as_a_multiset_and_first_column_first():
    g = np.random.default_rng(4)
    x = g.integers(0, 6, size=(4, 300)).astype(np.float32)                 # many exact ties
    idx, val, _, _ = T.rows_topk(x, 32)
    tv = torch.from_numpy(x).topk(32, dim=1).values.numpy()
    assert np.array_equal(np.sort(val, axis=1), np.sort(tv, axis=1))        # the same values, whichever columns torch took
    for r in range(4):
        assert np.array_equal(val[r], x[r, idx[r]])
        keys = [(-float(v), int(i)) for v, i in zip(val[r], idx[r])]
        assert keys == sorted(keys) and len(set(idx[r].tolist())) == 32     # descending, ties ascending by column, no column twice
        assert np.array_equal(idx[r], np.argsort(-x[r], kind="stable")[:32])


def test_model_special_values():
    inf, nan = np.inf, np.nan
    x = np.array([[1.0, -inf, nan, 3.0, -inf, 3.0],
                  [nan, nan, nan, nan, -inf, nan],
                  [nan, nan, nan, nan, nan, nan]], dtype=np.float32)
    idx, val, prob, lse = T.rows_topk(x, 5, "softmax")
    assert idx.tolist() == [[3, 5, 0, 1, 4], [4, -1, -1, -1, -1], [-1, -1, -1, -1, -1]]
    assert val[0].tolist() == [3.0, 3.0, 1.0, -inf, -inf] and np.all(np.isneginf(val[1:]))
    assert lse[1] == -inf and lse[2] == -inf and np.all(prob[1:] == 0.0) and np.all(prob[0, 3:] == 0.0)
    np.testing.assert_allclose(lse[0], np.log(2 * np.exp(3.0) + np.exp(1.0)), rtol=1e-14)
    np.testing.assert_allclose(prob[0, :3].sum(), 1.0, rtol=1e-14)
    assert T.rows_topk(x, 2, "sigmoid")[2][0].tolist() == [1 / (1 + np.exp(-3.0))] * 2
    big = np.array([[80.0, -80.0, 79.0]], dtype=np.float32)                 # no overflow at +-80
    _, _, p, l = T.rows_topk(big, 3, "softmax")
    assert np.isfinite(l[0]) and abs(l[0] - (80 + np.log1p(np.exp(-1.0) + np.exp(-160.0)))) < 1e-12 and p[0, 2] == np.exp(-80.0 - l[0])


# ---- the rounding model: the kernel's order in float32 stays inside the allowance, on the rows that load it most ---------------------
def _model_rows():
    g = np.random.default_rng(11)
    rows = {}
    for Cn in (1, 5, 257, 1025, 3129, 30522):
        rows[f"normal_{Cn}"] = g.standard_normal(Cn).astype(np.float32) * 3
        rows[f"ascending_{Cn}"] = np.linspace(-80, 80, Cn, dtype=np.float32)          # every column raises the running maximum
        rows[f"descending_{Cn}"] = np.linspace(80, -80, Cn, dtype=np.float32)
        rows[f"equal_{Cn}"] = np.full(Cn, 1.5, dtype=np.float32)                      # s = C exactly representable: the sum's own rounding
    r = g.standard_normal(1025).astype(np.float32)
    r[::7] = -np.inf
    r[3::11] = np.nan
    rows["inf_nan_1025"] = r
    rows["pm80_1025"] = np.where(np.arange(1025) % 2 == 0, 80.0, -80.0).astype(np.float32)
    return rows


def test_rounding_model_covers_the_kernels_summation_order():
    worst = 0.0
    for name, row in _model_rows().items():
        got, ref, allow = T.kernel_lse_f32(row), T.lse_row(row), T.lse_allowance(row)
        assert np.isfinite(ref) and allow > 0, name
        ratio = abs(got - ref) / allow
        assert ratio <= 1.0, (name, got, ref, allow)
        worst = max(worst, ratio)
    assert worst > 0.0                                                     # (the float32 order does round: the model is exercised)
    none = np.array([np.nan, -np.inf, -np.inf], dtype=np.float32)
    assert T.kernel_lse_f32(none) == -np.inf and T.lse_row(none) == -np.inf and T.lse_allowance(none) == 0.0


def test_allowance_grows_with_the_rows_spread_and_length_only():
    a = np.linspace(-1, 1, 1024, dtype=np.float32)
    assert T.lse_allowance(a * 80) > T.lse_allowance(a) and T.steps(30522) == 30 * 4 + 11 and T.steps(1) == 4 + 11
    assert T.lse_allowance(np.linspace(-80, 80, 30522)) < 2e-3             # the loosest row of the suite: still 1e-5 of the values' range


# ---- the compiler's assembly -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "topk.s")
        r = subprocess.run(["hipcc", *FLAGS, SRC, "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(dst).read()


def test_topk_kernels_are_present_and_use_no_scratch(isa):
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    names = " ".join(n for n, _ in sizes)
    for k in KERNELS:
        assert k in names, k
    spilled = [(n[:80], int(s)) for n, s in sizes if int(s) != 0]
    assert not spilled, spilled


def test_no_atomics_in_the_file(isa):
    for word in ("global_atomic", "flat_atomic", "cmpswap", "ds_add_f32", "ds_add_rtn_f32", "buffer_atomic"):
        assert word not in isa, word


def test_rows_are_read_with_16_byte_loads(isa):
    assert "global_load_dwordx4" in isa


# ---- argument checks of rmcl_rows_topk: they precede the launch, host buffers do ------------------------------------------------------
def test_rows_topk_rejects_bad_arguments_before_any_launch():
    import rmcl_pkg  # noqa: F401
    from rmcl_amd import _lib as L
    lib = L.lib
    x = (C.c_float * 64)(*([7.0] * 64))
    idx = (C.c_int32 * 64)(*([-7] * 64))
    val = (C.c_float * 64)(*([-7.0] * 64))
    prob = (C.c_float * 64)(*([-7.0] * 64))
    lse = (C.c_float * 64)(*([-7.0] * 64))

    def call(x_=x, ld=8, R=2, Cn=8, k=2, mode=L.TOPK_SOFTMAX, idx_=idx, val_=val):
        return lib.rmcl_rows_topk(x_, C.c_int64(ld), R, Cn, k, mode, idx_, val_, prob, lse, None)

    bad = [dict(x_=None), dict(idx_=None), dict(val_=None), dict(mode=3), dict(mode=-1), dict(Cn=0, k=1), dict(k=0), dict(k=9), dict(k=33, Cn=40, ld=40),
           dict(ld=7), dict(R=-1), dict(x_=C.cast(C.addressof(x) + 2, C.c_void_p))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"rows_topk" in lib.rmcl_last_error(), kw
    assert call(x_=None) == -1 and b"NULL" in lib.rmcl_last_error()
    assert call(R=0) == 0                                                   # no rows: no launch, nothing written
    for buf in (idx, val, prob, lse):
        assert all(v == -7 for v in buf)
    assert [v for v in x] == [7.0] * 64
    assert L.TOPK_MAX == 32 and "rmcl_rows_topk" in L.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rmcl.h")).read()
    for name, v in (("RMCL_TOPK_MAX", L.TOPK_MAX), ("RMCL_TOPK_RAW", L.TOPK_RAW), ("RMCL_TOPK_SOFTMAX", L.TOPK_SOFTMAX), ("RMCL_TOPK_SIGMOID", L.TOPK_SIGMOID)):
        assert re.search(rf"#define {name} {v}\b", hdr), name
