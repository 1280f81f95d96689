"""-m gpu: the streaming form of the k-split skinny fp32 GEMM (rmcl_tune_set key 6 at its default; csrc/gemm_exact.hip
gemm_skinny_stream_kernel) against the k-split kernel it re-times (key 6 = 1), bit for bit, and against fp64 with the bound of the
existing skinny tests.  The two forms promise the same arithmetic per output element - the same K / NW chunk per wave, the same 16-k
steps, the same MFMA order, the same sum over the waves, the same epilogue expressions - so every output must be torch.equal.

Shapes: the smallest at which an arm of the new form can go wrong.
  M   1, 16, 17, 32, 33, 48, 64, 70, 130: every RT (1, 2 and 4 row tiles per workgroup: RT divides ceil(M / 16)), a partial last row
      tile, more than one workgroup row (grid.y > 1 from 17 on with RT = 1, and at 130 with any RT).
  N, K  (16, 128): 2 steps per wave - a chunk shorter than the A ring, single-step bursts only; (40, 256): N no multiple of 16, one
      4-step burst; (128, 768), (768, 768), (3072, 768): the 12-step burst of 4 waves, few and many column tiles (RT 1 / 4);
      (768, 2048): the first K with 8 waves, 16 steps = a 12-step and a 4-step burst; (768, 3072): the 24-step burst ([K][N] weights:
      two of 12); (768, 6144): 48 steps, the multi-burst loop.
Both weight layouts ([N][K] and [K][N]) and the epilogues of the cls-only tail and the heads."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, gemm, stream  # noqa: E402

EPI_BIAS, EPI_GELU, EPI_SAVE_PREACT, EPI_RESIDUAL, EPI_DGELU, EPI_ACCUM, EPI_TANH, EPI_DUP = 1, 2, 4, 8, 16, 64, 128, 8192
MS = (1, 16, 17, 32, 33, 48, 64, 70, 130)
NKS = ((16, 128), (40, 256), (128, 768), (768, 768), (768, 2048), (768, 3072), (3072, 768), (768, 6144))
MMAX = max(MS)
AUX_ROWS = 3                                       # the residual is read in place at row stride AUX_ROWS * N (the tail: N_tokens * D)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def bits(t):
    return t.contiguous().view(torch.int32)


class Form:
    """rmcl_tune_set key 6 (process-global) around a region; the default comes back on the way out."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        check(lib.rmcl_tune_set(6, self.v), "tune_set")

    def __exit__(self, *exc):
        check(lib.rmcl_tune_set(6, -1), "tune_set")


gelu = lambda t: 0.5 * t * (1 + torch.erf(t / 2 ** 0.5))
dgelu = lambda t: 0.5 * (1 + torch.erf(t / 2 ** 0.5)) + t * torch.exp(-0.5 * t * t) / (2 * torch.pi) ** 0.5


def epilogues(M, N, W_arg, b_kc, X, bias, res, u, base):
    """The five launches of one (M, layout): {name: [outputs]} under the CURRENT key 6."""
    g = lambda **kw: gemm(X, W_arg, M, N, X.shape[1], 1, b_kc, L.F32, L.F32, **kw)
    out = {}
    out["gelu_preact"] = list(g(bias=bias, epi=EPI_BIAS | EPI_GELU | EPI_SAVE_PREACT, want_c2=True))
    out["residual_in_place"] = [g(bias=bias, aux=res, ld_aux=AUX_ROWS * N, epi=EPI_BIAS | EPI_RESIDUAL)]
    out["dgelu"] = [g(aux=u, ld_aux=N, epi=EPI_DGELU)]
    out["tanh_dup"] = list(g(bias=bias, epi=EPI_BIAS | EPI_TANH | EPI_DUP, want_c2=True))
    out["accum"] = [g(epi=EPI_ACCUM, C_init=base[:M])]
    return out


def operands(N, K):
    """Inputs for MMAX rows and the fp64 references of the five launches, computed once and sliced per M."""
    Xall, W, bias = rnd(MMAX, K, seed=1), rnd(N, K, seed=2, scale=0.05), rnd(N, seed=3)
    Wn = W.t().contiguous()                                                      # [K][N]
    res_all = rnd(MMAX, AUX_ROWS, N, seed=7)                                     # row m of the residual: res_all[m, 0]
    u_all, base_all = rnd(MMAX, N, seed=9), rnd(MMAX, N, seed=10)
    acc64 = Xall.double() @ W.double().t()
    pre64 = acc64 + bias.double()
    ref = {"gelu_preact": [gelu(pre64), pre64], "residual_in_place": [pre64 + res_all[:, 0].double()], "dgelu": [acc64 * dgelu(u_all.double())],
           "tanh_dup": [torch.tanh(pre64), torch.tanh(pre64)], "accum": [acc64 + base_all.double()]}
    return Xall, W, Wn, bias, res_all, u_all, base_all, ref


@pytest.mark.parametrize("N,K", NKS)
def test_streaming_form_has_the_ksplit_kernels_bits(N, K):
    Xall, W, Wn, bias, res_all, u_all, base_all, ref = operands(N, K)
    worst = 0.0
    for M in MS:
        X, res, u = Xall[:M].contiguous(), res_all[:M].contiguous(), u_all[:M].contiguous()
        for b_kc, W_arg in ((1, W), (0, Wn)):
            with Form(1):
                old = epilogues(M, N, W_arg, b_kc, X, bias, res, u, base_all)
            new = epilogues(M, N, W_arg, b_kc, X, bias, res, u, base_all)        # key 6 = -1: the streaming form
            for name, outs in new.items():
                for i, t in enumerate(outs):
                    assert torch.equal(bits(t), bits(old[name][i])), (M, N, K, b_kc, name, i)
                    e = rel_err(t, ref[name][i][:M])
                    worst = max(worst, e)
                    assert e < 2e-5, (M, N, K, b_kc, name, i, e)
    with Form(2):                                                                # 2 names the default form
        two = epilogues(MMAX, N, W, 1, Xall, bias, res_all, u_all, base_all)
    dflt = epilogues(MMAX, N, W, 1, Xall, bias, res_all, u_all, base_all)
    assert all(torch.equal(bits(a), bits(b)) for name in two for a, b in zip(two[name], dflt[name]))
    print(f"N {N} K {K}: largest rel. error against fp64 over all M, layouts and epilogues {worst:.2e}")


@pytest.mark.parametrize("N,K", ((16, 128), (40, 256), (128, 768)))
def test_row_split_kernel_runs_the_same_epilogues_within_the_fp64_bound(N, K):
    """Key 6 = 0: gemm_skinny_kernel (every wave its own 16 rows, four accumulator chains summed at the end), which shares
    skinny_epilogue with the k-split kernel but loads the tail's operands at the point of use.  It sums in another order, so no bit
    equality with the other forms is claimed: the five launches against fp64 with this file's bound."""
    Xall, W, Wn, bias, res_all, u_all, base_all, ref = operands(N, K)
    worst = 0.0
    for M in (1, 17, 64, 70):
        X, res, u = Xall[:M].contiguous(), res_all[:M].contiguous(), u_all[:M].contiguous()
        for b_kc, W_arg in ((1, W), (0, Wn)):
            with Form(0):
                got = epilogues(M, N, W_arg, b_kc, X, bias, res, u, base_all)
            for name, outs in got.items():
                for i, t in enumerate(outs):
                    e = rel_err(t, ref[name][i][:M])
                    worst = max(worst, e)
                    assert e < 2e-5, (M, N, K, b_kc, name, i, e)
    print(f"row-split N {N} K {K}: largest rel. error against fp64 over all M, layouts and epilogues {worst:.2e}")


def rows_bf16(A, Wt, M, N, K, lda, bias=None, aux=None, ld_aux=0, epi=0):
    out = torch.zeros(M, N, device=DEV)
    rc = lib.rmcl_gemm_rows_bf16(P(A), P(Wt), P(out), None, P(bias), P(aux), M, N, K, I64(lda), N, ld_aux, epi, stream())
    return rc, out


@pytest.mark.parametrize("M", [3, 32, 64])
def test_bf16_rows_read_in_place_equal_gather_then_fp32_form(M):
    """A = the cls rows of a bf16 [M * 185, 768] tensor at row stride 185 * 768 (the tail's proj): the bits of rmcl_rows_gather_f32
    followed by the fp32 GEMM, in the k-split form and in the streaming form."""
    NT, D = 185, 768
    A = rnd(M * NT, D, seed=21).to(torch.bfloat16)
    for N in (768, 128):
        W, bias, res = rnd(N, D, seed=22, scale=0.05), rnd(N, seed=23), rnd(M, AUX_ROWS, N, seed=24)
        rows = torch.full((M, D), float("nan"), device=DEV)
        check(lib.rmcl_rows_gather_f32(P(A), L.BF16, P(rows), M, D, I64(NT), I64(0), stream()), "rows_gather_f32")
        assert torch.equal(rows, A.view(M, NT, D)[:, 0].float())
        for kw in (dict(), dict(bias=bias, aux=res, ld_aux=AUX_ROWS * N, epi=EPI_BIAS | EPI_RESIDUAL)):
            with Form(1):
                want = gemm(rows, W, M, N, D, 1, 1, L.F32, L.F32, **kw)
                rc, _ = rows_bf16(A, W, M, N, D, NT * D, **kw)
                assert rc != 0 and b"bf16" in lib.rmcl_last_error()              # the k-split kernel has no such operand: refused, not converted
            assert torch.equal(bits(gemm(rows, W, M, N, D, 1, 1, L.F32, L.F32, **kw)), bits(want))
            rc, got = rows_bf16(A, W, M, N, D, NT * D, **kw)
            check(rc, "gemm_rows_bf16")
            assert torch.equal(bits(got), bits(want)), (M, N, kw.get("epi", 0))
            ref = rows.double() @ W.double().t() + ((bias.double() + res[:, 0].double()) if kw else 0)
            assert rel_err(got, ref) < 2e-5
    # shapes the streaming kernel does not run are refused for this operand
    rc, _ = rows_bf16(A, rnd(64, 48, seed=1), M, 64, 48, NT * D)
    assert rc != 0
