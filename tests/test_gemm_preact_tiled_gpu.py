"""-m gpu: the tiled pre-activation stash of the 192x384 kernel (gemm_sw.hip, EPI_PREACT_TILED) against the row-major stash it replaces.
One chain is fc1 (h = gelu(u), u stashed) then fc2-dX (du = (dx W2) * gelu'(u)); it runs once with the row-major stash and once with the
tiled one on the same seeded bf16 operands.  The two forms do the same operations on the same values in the same order, so h and du are
compared as RAW BITS.  The tiled buffer starts as NaN bit patterns - a block or fragment fc1 fails to write shows in du - and carries a
guard region behind its last block; outputs carry a sentinel and guard rows behind M.  Every tiled chain runs three times and must repeat
its bits: a misplaced wait shows as a difference between repeats."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream  # noqa: E402

EPI_BIAS, EPI_GELU, EPI_SAVE_PREACT, EPI_DGELU, EPI_DROPOUT, EPI_DROP_BWD, EPI_TILED = 1, 2, 4, 16, 512, 1024, 16384
MS = [1, 97, 185, 192, 193, 370]      # one partial tile; both wave groups partly dead; rows per sample; the exact tile; two row tiles, uneven (rows_per_tile != 192)
NS = [384, 768, 1536]                 # one column tile; the tiles_n % 4 != 0 order; the band order
KS = [128, 192, 768]                  # no steady-state k-tile; exactly one; the step's
M_MAX, N_MAX, K_MAX, GUARD, TGUARD = 370, 1536, 768, 4, 4096


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@pytest.fixture(scope="module")
def data():
    """Seeded operands, made once at the largest shape; a case takes the leading rows / columns."""
    return {"X": rnd(M_MAX, K_MAX, seed=1).to(torch.bfloat16), "W1": rnd(N_MAX, K_MAX, seed=2, scale=0.05).to(torch.bfloat16),
            "b1": rnd(N_MAX, seed=3, scale=0.5), "DX": rnd(M_MAX, K_MAX, seed=4).to(torch.bfloat16),
            "W2T": rnd(N_MAX, K_MAX, seed=5, scale=0.05).to(torch.bfloat16),
            # the folded form: row partials of the LayerNorm input, per-column s / c
            "part": rnd(M_MAX, 16, 2, seed=6).abs() * 50.0 + 1.0, "s": rnd(N_MAX, seed=7, scale=0.3), "c": rnd(N_MAX, seed=8, scale=0.3)}


class Tune:
    """rmcl_tune_set key 0 = 70 asks for the 192x384 kernel at any shape it supports (process-global: restored on the way out)."""

    def __enter__(self):
        check(lib.rmcl_tune_set(0, 70), "tune_set")

    def __exit__(self, *exc):
        check(lib.rmcl_tune_set(0, -1), "tune_set")


def tiled_elems(M, N):
    return (M + 191) // 192 * (N // 384) * 192 * 384


def sentinel(M, N):
    return torch.full((M + GUARD, N), 7.0, dtype=torch.bfloat16, device=DEV)


def stash_buffer(M, N, tiled):
    if not tiled:
        return sentinel(M, N)
    u = torch.full((tiled_elems(M, N) + TGUARD,), float("nan"), dtype=torch.bfloat16, device=DEV)
    u[tiled_elems(M, N):] = 7.0
    return u


def chain(data, M, N, K, tiled, folded=False, drop=False):
    """fc1 then fc2-dX through rmcl_gemm (folded fc1: rmcl_linear_lnfold); returns (h, du) with their guard rows and the stash."""
    flag = EPI_TILED if tiled else 0
    X, W1, b1 = data["X"][:M, :K].contiguous(), data["W1"][:N, :K].contiguous(), data["b1"][:N].contiguous()
    DX, W2T = data["DX"][:M, :K].contiguous(), data["W2T"][:N, :K].contiguous()
    h, du, u = sentinel(M, N), sentinel(M, N), stash_buffer(M, N, tiled)
    if folded:
        nparts = 4 * (K // 192)
        part, s, c = data["part"][:M, :nparts].contiguous(), data["s"][:N].contiguous(), data["c"][:N].contiguous()
        check(lib.rmcl_linear_lnfold(P(X), P(W1), P(s), P(c), P(part), nparts, P(h), P(u), M, N, K, 1 | (2 if tiled else 0), F(1e-6), None, None,
                                     stream()), "linear_lnfold")
    else:
        e1 = EPI_BIAS | EPI_GELU | EPI_SAVE_PREACT | (EPI_DROPOUT if drop else 0) | flag
        assert lib.rmcl_gemm_route(M, N, K, e1, L.BF16, 1, 1) == 2
        check(lib.rmcl_gemm(P(X), P(W1), P(h), P(u), P(b1), None, M, N, K, I64(K), I64(K), N, 0, F(1.0), e1, 1, L.BF16, L.BF16, 1, 1, 0, stream()), "fc1")
    e2 = EPI_DGELU | (EPI_DROP_BWD if drop else 0) | flag
    assert lib.rmcl_gemm_route(M, N, K, e2, L.BF16, 1, 1) == 2
    check(lib.rmcl_gemm(P(DX), P(W2T), P(du), None, None, P(u), M, N, K, I64(K), I64(K), N, N, F(1.0), e2, 1, L.BF16, L.BF16, 1, 1, 0, stream()), "fc2dx")
    return h, du, u


def bits(t):
    return t.view(torch.int16)


def ab(data, M, N, K, **kw):
    what = f"M={M} N={N} K={K} {kw}"
    with Tune():
        new = [chain(data, M, N, K, True, **kw) for _ in range(3)]
        old = chain(data, M, N, K, False, **kw)
    torch.cuda.synchronize()
    for r in new[1:]:
        for i in range(3):                                         # h, du and the tiled buffer itself (dead rows included: same values every run)
            assert torch.equal(bits(new[0][i]), bits(r[i])), (what, "repeat", i)
    h, du, u = new[0]
    for i, (x, y) in enumerate(((h, old[0]), (du, old[1]))):       # live rows, guard rows and sentinel alike
        assert torch.equal(bits(x), bits(y)), (what, "h du"[2 * i:2 * i + 2], int((bits(x) != bits(y)).sum()))
    assert bool(torch.isfinite(h[:M].float()).all()) and bool(torch.isfinite(du[:M].float()).all()), what
    assert bool((h[M:].float() == 7.0).all()) and bool((du[M:].float() == 7.0).all()), what
    assert bool((u[tiled_elems(M, N):].float() == 7.0).all()), what
    assert bool((old[2][M:].float() == 7.0).all()), what
    return new[0], old


@pytest.mark.parametrize("M", MS)
def test_chain_bits(data, M):
    for N in NS:
        for K in KS:
            ab(data, M, N, K)


def test_tiled_stash_holds_the_row_major_values(data):
    """Every live element of the row-major stash is somewhere in its tile's block (a permutation inside the block, not across blocks)."""
    M, N, K = 370, 768, 192
    (h, du, u), old = ab(data, M, N, K)
    rows = (M + 1) // 2                                            # rows_per_tile of two row tiles
    for tr in range(2):
        for tc in range(N // 384):
            blk = u[(tr * (N // 384) + tc) * 192 * 384:][:192 * 384]
            ref = old[2][tr * rows:min(M, (tr + 1) * rows), tc * 384:(tc + 1) * 384]
            assert bool(torch.isin(bits(ref).flatten().unique(), bits(blk)).all()), (tr, tc)


@pytest.mark.parametrize("M", [97, 370])
def test_folded_fc1_chain_bits(data, M):
    for K in (192, 768):
        ab(data, M, 768, K, folded=True)


def test_dropout_pair_bits(data):
    ab(data, 193, 768, 192, drop=True)


def test_shapes_the_kernel_cannot_take_are_refused(data):
    M, K = 193, 192
    X, W = data["X"][:M, :K].contiguous(), data["W1"][:384, :K].contiguous()
    u = stash_buffer(M, 384, True)
    e1 = EPI_BIAS | EPI_GELU | EPI_SAVE_PREACT | EPI_TILED
    with Tune():
        # N = 192: no 384-column tile
        out = sentinel(M, 192)
        rc = lib.rmcl_gemm(P(X), P(W), P(out), P(u), P(data["b1"]), None, M, 192, K, I64(K), I64(K), 192, 0, F(1.0), e1, 1, L.BF16, L.BF16, 1, 1, 0, stream())
        assert rc != 0 and b"EPI_PREACT_TILED" in lib.rmcl_last_error()
        # fp32 output
        out32 = torch.full((M + GUARD, 384), 7.0, device=DEV)
        rc = lib.rmcl_gemm(P(X), P(W), P(out32), P(u), P(data["b1"]), None, M, 384, K, I64(K), I64(K), 384, 0, F(1.0), e1, 1, L.BF16, L.F32, 1, 1, 0, stream())
        assert rc != 0 and b"EPI_PREACT_TILED" in lib.rmcl_last_error()
        # [K][cols] weights on the consumer
        out = sentinel(M, 384)
        rc = lib.rmcl_gemm(P(X), P(W), P(out), None, None, P(u), M, 384, K, I64(K), I64(384), 384, 384, F(1.0), EPI_DGELU | EPI_TILED, 1, L.BF16, L.BF16, 1, 0, 0,
                           stream())
        assert rc != 0 and b"EPI_PREACT_TILED" in lib.rmcl_last_error()
    # default routing: the shape does not reach the 192x384 kernel, so the flag is refused, not dropped
    out = sentinel(M, 384)
    rc = lib.rmcl_gemm(P(X), P(W), P(out), P(u), P(data["b1"]), None, M, 384, K, I64(K), I64(K), 384, 0, F(1.0), e1, 1, L.BF16, L.BF16, 1, 1, 0, stream())
    assert rc != 0 and b"EPI_PREACT_TILED" in lib.rmcl_last_error()
    torch.cuda.synchronize()
    assert bool((out.float() == 7.0).all()) and bool((out32 == 7.0).all()) and bool(torch.isnan(u[:tiled_elems(M, 384)].float()).all())
