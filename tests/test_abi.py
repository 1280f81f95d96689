"""CPU: the C-ABI library loads and exports every symbol include/rmcl.h declares (no compute calls)."""
import os
import re

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rmcl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rmcl_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported():
    syms = declared_symbols()
    assert len(syms) >= 25
    missing = [s for s in syms if not hasattr(_lib.lib, s)]
    assert not missing, missing
    assert sorted(_lib.EXPORTS) == syms


def test_version_and_layout_are_host_only_calls():
    import ctypes as C
    assert _lib.lib.rmcl_version() == 1
    d = _lib.Dims(B=2, L=40, P=144, D=768, H=12, layers=12, mlp=3072, patch_k=3072, proj=128, vocab=30522, dtype=0, exact=1)
    lay = _lib.Layout()
    _lib.lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    # 112 285 440 trainable parameters of ViLT-B/32 + heads plus <=63 pad elements per tensor
    n_tensors = 10 + 12 * 12 + 2 + 5 + 2 + 2
    exact = 112285440 + 2 * 768 + 2                                  # + itm head (not in the SURVEY count)
    assert exact <= lay.total <= exact + 64 * n_tensors
    assert lay.ema_end == lay.pool_w < lay.itm_w < lay.total and lay.ema_end == 111694848
    assert _lib.lib.rmcl_stash_bytes(C.byref(d), _lib.MODE_FULL) > _lib.lib.rmcl_stash_bytes(C.byref(d), _lib.MODE_DATA) > 0
    assert _lib.lib.rmcl_stash_bytes(C.byref(d), _lib.MODE_INFER) == 256


def test_argument_errors_are_reported_not_crashed():
    import ctypes as C
    rc = _lib.lib.rmcl_gemm(None, None, None, None, None, None, 1, 1, 1, C.c_int64(1), C.c_int64(1), 1, 1,
                            C.c_float(1.0), 0, 1, 0, 0, 1, 1, 1, None)
    assert rc == -1
    assert b"NULL" in _lib.lib.rmcl_last_error()


def test_attention_scratch_holds_the_fused_kernels_row_statistics():
    """The fused forward writes B * H * NKP fp32 log-sum-exp values (NKP = 64 / 128 for N <= 64 / 128) into a bf16 `probs` of
    rmcl_attention_scratch_elems elements, the two-kernel backward as many fp32 deltas into `scores`: at least 2 * B * H * NKP elements,
    which N * ldp alone misses for N <= 8.  The matrices of the unfused path dominate from N = 9 on: the engine's arenas keep their sizes."""
    import ctypes as C
    elems = _lib.lib.rmcl_attention_scratch_elems
    for B, H in ((2, 12), (3, 1)):
        for N in (1, 7, 8, 9, 64, 65):
            assert elems(B, H, N) >= 2 * B * H * (64 if N <= 64 else 128), (B, H, N)
            assert elems(B, H, N) >= B * H * N * ((N + 7) // 8 * 8)
        for N in (9, 12, 42, 128, 129, 185, 256, 281, 512):
            assert elems(B, H, N) == B * H * N * ((N + 7) // 8 * 8), (B, H, N)
    # default dims (L = 40, P = 144: N = 185), fp32 exact and bf16: workspace, DATA stash, FULL stash - what the three functions returned
    # at c554b75, the last commit with the plain B * H * N * ldp sizing (at N = 185 the new expression is that same product)
    pinned = {(0, 2): (99864832, 178776128, 260614208), (0, 64): (1822274816, 5720732416, 8339550976),
              (1, 2): (78394624, 103757888, 144676928), (1, 64): (1135228160, 3320148736, 4629558016)}
    for (dt, B), want in pinned.items():
        d = _lib.Dims(B=B, L=40, P=144, D=768, H=12, layers=12, mlp=3072, patch_k=3072, proj=128, vocab=30522, dtype=dt, exact=1 - dt)
        got = (_lib.lib.rmcl_workspace_bytes(C.byref(d)), _lib.lib.rmcl_stash_bytes(C.byref(d), _lib.MODE_DATA),
               _lib.lib.rmcl_stash_bytes(C.byref(d), _lib.MODE_FULL))
        assert got == want, (dt, B, got)
