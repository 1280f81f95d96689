"""CPU: every entry point include/rmcl.h declares is named by at least one test, and the NULL checks of the public wrappers.

The coverage guard is textual on purpose: it cannot tell a good test from a bad one, but it does notice an exported function that
no test file mentions at all - the state the word-patch-alignment, ITM-head and arena kernels were in before
tests/test_wpa_kernels_gpu.py.  The exempt list may only shrink: a listed name that IS mentioned by a test fails the guard too."""
import ctypes as C
import glob
import os
import re

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points no test file names, one reason each
EXEMPT = {
    "rmcl_l2_prefetch_experiment": "measurement experiment (tools/l2_prefetch_bench.py); writes nothing but time stamps, not used by any pass",
    "rmcl_prof_begin": "hipEvent timing of GEMM launches for bench.py's roofline object; no numerical result to pin",
    "rmcl_prof_end": "second half of rmcl_prof_begin",
    "rmcl_set_prefetch_stream": "stream of the stash-prefetch experiment (tune key 12, off by default)",
}


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rmcl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rmcl_[a-z0-9_]+)\s*\(", text)))


def test_every_exported_entry_point_is_named_by_a_test():
    syms = declared_symbols()
    assert len(syms) >= 80 and sorted(_lib.EXPORTS) == syms
    me = os.path.abspath(__file__)
    text = "\n".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) if os.path.abspath(f) != me)
    named = {s for s in syms if re.search(r"\b" + s + r"\b", text)}
    assert not set(EXEMPT) - set(syms), "exempt names that the header no longer declares"
    uncovered = sorted(set(syms) - named - set(EXEMPT))
    assert not uncovered, f"exported but named by no test: {uncovered}"
    stale = sorted(set(EXEMPT) & named)
    assert not stale, f"exempt but now named by a test (drop them from EXEMPT): {stale}"


def _rejected(rc, what):
    assert rc == -1, what
    msg = _lib.lib.rmcl_last_error()
    assert msg and b"NULL" in msg and what.encode() in msg, (what, msg)


def test_null_operands_are_rejected_before_any_launch():
    """The argument check precedes the launch, so these calls need no GPU: each must return -1 with a message that names the entry
    point and the NULL operand.  The buffers handed over are host memory; a wrapper that got past its check would launch on them."""
    lib = _lib.lib
    buf = (C.c_float * 16)()
    ibuf = (C.c_int32 * 16)()
    n, f = C.c_int64(4), C.c_float
    _rejected(lib.rmcl_cast_f32(None, buf, _lib.F32, n, None), "cast")
    _rejected(lib.rmcl_cast_f32(buf, None, _lib.BF16, n, None), "cast")
    _rejected(lib.rmcl_add_cast_f32(None, None, None, buf, _lib.F32, n, None), "add_cast")
    _rejected(lib.rmcl_add_cast_f32(buf, buf, buf, None, _lib.F32, n, None), "add_cast")
    _rejected(lib.rmcl_delta_channel_norm(None, buf, C.c_int64(1), 3, 4, None), "delta_channel_norm")
    _rejected(lib.rmcl_delta_channel_norm(buf, None, C.c_int64(1), 3, 4, None), "delta_channel_norm")
    # dsim = -w[b] * T^T reads w: a given dsim requires w; the inference call (dsim NULL) does not
    _rejected(lib.rmcl_wpa_distance(buf, buf, None, buf, buf, 1, 1, 1, 4, None), "wpa_distance")
    _rejected(lib.rmcl_wpa_distance(None, buf, buf, buf, None, 1, 1, 1, 4, None), "wpa_distance")
    _rejected(lib.rmcl_wpa_distance(buf, None, buf, buf, None, 1, 1, 1, 4, None), "wpa_distance")
    _rejected(lib.rmcl_wpa_distance(buf, buf, buf, None, None, 1, 1, 1, 4, None), "wpa_distance")
    _rejected(lib.rmcl_wpa_cost_finish(None, ibuf, ibuf, 1, 1, 1, 4, None), "wpa_cost_finish")
    _rejected(lib.rmcl_ipot_f32(buf, ibuf, ibuf, None, 1, 1, 1, 4, f(0.5), 50, None), "ipot")
    _rejected(lib.rmcl_l2norm_rows_fwd(buf, buf, None, 1, 4, f(1e-5), None), "l2norm_rows_fwd")
    _rejected(lib.rmcl_l2norm_rows_bwd(buf, buf, buf, None, 1, 4, None), "l2norm_rows_bwd")
    _rejected(lib.rmcl_itm_fwd(buf, buf, buf, None, buf, None, None, 1, 4, f(1.0), None), "itm_fwd")
    _rejected(lib.rmcl_itm_bwd(buf, buf, buf, None, None, None, 1, 4, f(1.0), None), "itm_bwd")
    _rejected(lib.rmcl_ln_fold(None, buf, buf, buf, None), "ln_fold")
    _rejected(lib.rmcl_weight_transpose_bf16(None, buf, buf, None), "weight_transpose")


def test_heads_arguments_are_rejected_before_any_launch():
    """rmcl_heads_forward2 / rmcl_heads_backward: every required operand as NULL, an unknown flag bit, and a backward with neither dq nor
    dcls_extra.  Host buffers throughout, as above."""
    lib = _lib.lib
    buf = (C.c_float * 16)()
    d = _lib.Dims(B=1, L=4, P=3, D=64, H=1, layers=1, mlp=64, patch_k=64, proj=64, vocab=64, dtype=_lib.F32, exact=1, Pp=3)
    dp = C.byref(d)
    fwd = [dp, buf, buf, buf, buf, buf, buf]                                     # d, pool32, head32, xn, hstash, cls_feats, q
    for i in (0, 1, 3, 4, 5):
        a = list(fwd)
        a[i] = None
        _rejected(lib.rmcl_heads_forward2(*a, 0, None), "heads_forward")
    assert lib.rmcl_heads_forward2(*fwd, 2, None) == -1
    assert b"heads_forward" in lib.rmcl_last_error() and b"unknown flag" in lib.rmcl_last_error()
    bwd = [dp, buf, buf, buf, buf, buf, buf, None, buf]                          # d, pool32, head32, hstash, dq, dcls_extra, dcls, grads32, workspace
    for i in (0, 1, 3, 6, 8):
        a = list(bwd)
        a[i] = None
        _rejected(lib.rmcl_heads_backward(*a, None), "heads_backward")
    a = list(bwd)
    a[4] = a[5] = None
    assert lib.rmcl_heads_backward(*a, None) == -1
    assert b"heads_backward" in lib.rmcl_last_error() and b"neither dq nor dcls_extra" in lib.rmcl_last_error()
