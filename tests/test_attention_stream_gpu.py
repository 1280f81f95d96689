"""-m gpu: rmcl_attention_stream_fwd / rmcl_attention_stream_bwd (csrc/attention_stream.hip) against float64, row by row.

Method, reference, metric and buffers are those of tests/test_attention_kernels_gpu.py, whose helpers are imported: Attention.forward in
float64 on the bf16-rounded inputs; the worst-row error of out, dQ, dK, dV; bound BF16_FACTOR (3) x rounding_model on the same case, kind
`one_kernel`: the streaming backward takes delta = rowsum(dO * bf16(O)) from the forward's output, as the one-kernel backward does.
Guarded, exactly sized, NaN-initialised buffers; inputs unchanged; no NaN out; dK / dV rows of masked keys exactly zero; every case that
is swept runs twice and must give the same bits.

The log-sum-exp (fp32 [B, H, NKP] in `probs`, NKP = rmcl_attention_stream_stat_elems / (B * H) = N rounded up to the 64-row block) is held
to LSE_TOL = 1e-4 on unit-normal input: at N = 512 the fp32 row sum of <= 512 terms adds 512 * 2^-24 = 3e-5 relative error to that file's
3e-5 (64-term score) + ulp terms.

Tiling of the launcher (what the N sweep straddles): keys and queries stream in blocks of 64 rows, the forward and the dq kernel give a
workgroup 64 queries, the dkv kernel 128 keys, a wave works on tiles of 16 rows.  So 64|65, 256|257, 320|321, 384|385 (also a 128-key
group), 448|449 are block / workgroup boundaries and 272|273 a tile boundary inside a block; 511|512 is the upper end.  There is one
instantiation of each kernel and no launch variant to compare.

The `late` mask is the leading-blocks-masked case: sample 0 has only keys >= N - 60 valid, sample 1 only the last key, so the running
maximum of the online softmax is still -inf when the first valid key arrives."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, stream  # noqa: E402
from tests.test_attention_kernels_gpu import (BF16_FACTOR, BLOCKS, E32, LSE_TOL, Case, Guarded, attention_autograd, bf, bits,  # noqa: E402
                                              figures, inputs, rounding_model, same_bits, split)

SWEEP_N = (257, 272, 273, 281, 320, 321, 384, 385, 448, 449, 511, 512, 1, 17, 64, 65, 185, 256)


def case_inputs(case):
    """fp32 qkv, dout and the int32 mask on the CPU: tests/test_attention_kernels_gpu.inputs, plus the `late` mask on the same data."""
    if case.mask != "late":
        return inputs(case)
    qkv, dout, _ = inputs(case._replace(mask="all"))
    m = torch.zeros(case.B, case.N, dtype=torch.int32)
    m[0, max(case.N - 60, 0):] = 1
    m[1:, case.N - 1] = 1
    return qkv, dout, m


def kernel_values(case):
    qkv, dout, mask = case_inputs(case)
    return bf(qkv), bf(dout), mask


@functools.lru_cache(maxsize=None)
def reference(case):
    return attention_autograd(*kernel_values(case), case.B, case.N, case.H, torch.float64)


@functools.lru_cache(maxsize=None)
def model_figures(case):
    return figures(rounding_model(*kernel_values(case), case.B, case.N, case.H, delta_from_O=True), reference(case)[0])


def stat_rows(B, H, N):
    ne = int(lib.rmcl_attention_stream_stat_elems(B, H, N))
    assert ne % (B * H) == 0 and ne // (B * H) >= N and 2 * ne <= int(lib.rmcl_attention_scratch_elems(B, H, N))   # fp32 in a bf16 `probs`
    return ne // (B * H)


def run_stream(case):
    """Forward + backward through the C ABI on guarded, exactly sized, NaN-initialised buffers."""
    B, N, H = case[:3]
    D = H * 64
    qkv_c, dout_c, mask_c = kernel_values(case)
    qkv, dout, mask = qkv_c.to(DEV, torch.bfloat16), dout_c.to(DEV, torch.bfloat16), mask_c.to(DEV)
    keep = (qkv.clone(), dout.clone(), mask.clone())
    ne = int(lib.rmcl_attention_scratch_elems(B, H, N))
    back = B * H * 256 * 4 + 4096
    nan = float("nan")
    bt = torch.bfloat16
    buf = {"out": Guarded(B * N * D, bt, back, nan), "dqkv": Guarded(B * N * 3 * D, bt, back, nan), "probs": Guarded(ne, bt, back, nan),
           "scores": Guarded(ne, torch.float32, back, nan), "dS": Guarded(ne, bt, back, nan)}
    t = {n: b.t for n, b in buf.items()}
    check(lib.rmcl_attention_stream_fwd(P(qkv), P(mask), P(t["out"]), P(t["probs"]), P(t["scores"]), B, N, H, stream()), "attention_stream_fwd")
    check(lib.rmcl_attention_stream_bwd(P(qkv), P(mask), P(t["probs"]), P(dout), P(t["out"]), P(t["dqkv"]), P(t["scores"]), P(t["dS"]),
                                        B, N, H, stream()), "attention_stream_bwd")
    torch.cuda.synchronize()
    for n, b in buf.items():
        assert b.intact(), f"{n}: guard bytes overwritten"
    assert torch.equal(bits(qkv), bits(keep[0])) and torch.equal(bits(dout), bits(keep[1])) and torch.equal(mask, keep[2])
    out, dqkv = t["out"].view(B * N, D).cpu(), t["dqkv"].view(B * N, 3 * D).cpu()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dqkv).any())
    nkp = stat_rows(B, H, N)
    res = split(out, dqkv, D)
    res["lse"] = buf["probs"].raw[Guarded.FRONT:Guarded.FRONT + B * H * nkp * 4].view(torch.float32).view(B, H, nkp)[:, :, :N].cpu()
    return res


def assert_parity(case, got):
    ref, lse_ref = reference(case)
    mod = model_figures(case)
    fig = figures(got, ref)
    bad = []
    for b in BLOCKS:
        allowed = BF16_FACTOR * (mod[b][0] + (0.0 if bool(ref[b].any()) else E32))   # (the zero-reference rule: N = 1, dQ = dK = 0)
        print(f"{tuple(case)} stream [one_kernel] {b}: worst row {fig[b][0]:.3e} (model {mod[b][0]:.3e}, allowed {allowed:.3e})  "
              f"global {fig[b][1]:.3e} (model {mod[b][1]:.3e})")
        if not fig[b][0] <= allowed:
            bad.append((b, fig[b][0], allowed))
    masked = (case_inputs(case)[2].reshape(-1) == 0)
    for b in ("dK", "dV"):
        assert bool((got[b][masked] == 0).all()), f"{b}: rows of masked keys are not exactly zero"
    if case.family == "normal":
        dl = float((got["lse"].double() - lse_ref).abs().max())
        print(f"{tuple(case)} stream lse: max |d| {dl:.3e}")
        assert dl <= LSE_TOL, f"log-sum-exp off by {dl}"
    assert not bad, bad


@pytest.mark.parametrize("N", SWEEP_N)
def test_n_sweep(N):
    """Unit-normal input, the hole mask, both sides of every block / workgroup / tile boundary of the launcher, the workload's 281 and the
    lengths the encoder does not route here; run twice: the same bits."""
    case = Case(2, N, 12, "holes", "normal")
    got = run_stream(case)
    assert_parity(case, got)
    assert same_bits(got, run_stream(case), BLOCKS + ("lse",)), "run-to-run difference"


@pytest.mark.parametrize("kind", ["holes", "tail", "key0", "text", "all", "late"])
@pytest.mark.parametrize("N", [281, 512])
def test_mask_shapes(N, kind):
    """Trailing key blocks masked, one valid key, the real batch's text-pad + image-pad pattern, no masked key, and `late`: every leading
    key block masked (sample 1: all but the last key)."""
    case = Case(2, N, 12, kind, "normal")
    assert_parity(case, run_stream(case))


@pytest.mark.parametrize("family", ["qx4", "v+3", "k+2"])
def test_stress_inputs(family):
    case = Case(2, 281, 12, "text", family)
    assert_parity(case, run_stream(case))


@pytest.mark.parametrize("H", [1, 3])
def test_head_counts(H):
    case = Case(2, 281, H, "holes", "normal")
    assert_parity(case, run_stream(case))


def test_three_samples():
    case = Case(3, 281, 12, "text", "normal")
    assert_parity(case, run_stream(case))


def test_statistics_rows_fit_the_scratch_sizing():
    for N in (1, 8, 9, 63, 64, 65, 128, 129, 192, 193, 256, 257, 281, 511, 512):
        assert stat_rows(2, 12, N) == (N + 63) // 64 * 64


@pytest.mark.parametrize("N", [0, 513])
def test_bad_n_is_rejected_before_anything_is_written(N):
    """N = 0 and N = 513 (and, at a valid N, every NULL argument) return non-zero with every byte of every buffer unchanged."""
    B, H, n = 1, 2, 512
    D = H * 64
    ne = int(lib.rmcl_attention_scratch_elems(B, H, n))
    bt = torch.bfloat16
    qkv = torch.randn(B * n, 3 * D, device=DEV).to(bt)
    dout = torch.randn(B * n, D, device=DEV).to(bt)
    mask = torch.ones(B, n, dtype=torch.int32, device=DEV)
    buf = {"out": Guarded(B * n * D, bt, 4096, 1.0), "dqkv": Guarded(B * n * 3 * D, bt, 4096, 1.0), "probs": Guarded(ne, bt, 4096, 1.0),
           "scores": Guarded(ne, torch.float32, 4096, 1.0), "dS": Guarded(ne, bt, 4096, 1.0)}
    before = {k: b.raw.clone() for k, b in buf.items()}
    keep = (qkv.clone(), dout.clone())
    t = {k: b.t for k, b in buf.items()}
    fwd = [P(qkv), P(mask), P(t["out"]), P(t["probs"]), P(t["scores"])]
    bwd = [P(qkv), P(mask), P(t["probs"]), P(dout), P(t["out"]), P(t["dqkv"]), P(t["scores"]), P(t["dS"])]
    assert lib.rmcl_attention_stream_fwd(*fwd, B, N, H, stream()) != 0
    assert lib.rmcl_attention_stream_bwd(*bwd, B, N, H, stream()) != 0
    for i in range(len(fwd)):
        a = list(fwd)
        a[i] = None
        assert lib.rmcl_attention_stream_fwd(*a, B, n, H, stream()) == -1 and b"NULL" in lib.rmcl_last_error()
    for i in range(len(bwd)):
        a = list(bwd)
        a[i] = None
        assert lib.rmcl_attention_stream_bwd(*a, B, n, H, stream()) == -1 and b"NULL" in lib.rmcl_last_error()
    torch.cuda.synchronize()
    for k, b in buf.items():
        assert torch.equal(b.raw, before[k]), f"{k} was written by a rejected call"
    assert torch.equal(bits(qkv), bits(keep[0])) and torch.equal(bits(dout), bits(keep[1]))
