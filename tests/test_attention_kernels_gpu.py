"""-m gpu: rmcl_attention_fwd / rmcl_attention_bwd against float64, row by row, at every tile-count arm of csrc/attention.hip.

Arms.  (bf16, exact = 0) with N <= 256 runs the fused kernels, instantiated for NKT = 4 / 8 / 12 / 16 key tiles at N <= 64 / 128 / 192 /
256; its backward is ONE kernel when `out` is given, rmcl_tune_set key 2 is 1 and N <= 192, and the two-kernel form otherwise.  exact = 1
(bf16 or fp32 storage) and every N > 256 run the unfused path: batched GEMM + softmax_fwd / softmax_bwd kernels, N <= 512.

Reference.  Attention.forward (QK^T * 0.125, key-padding mask as -inf, softmax, @ V) in float64 on the values the kernel reads (the
bf16-rounded qkv and dout on the bf16 arms); gradients by autograd.  Computed once per case on the CPU and shared.

Metric.  For out and for dQ, dK, dV (the column thirds of dqkv), per row of [B*N, H*64]:
  err = |got - ref|_2 / max(|ref|_2, 0.05 * rms row norm of the block), asserted on the MAXIMUM over rows
(a block whose reference is identically zero - N = 1: dQ = dK = 0 - is measured against the rms row norm of dV).  dK / dV rows of masked
keys must be exactly zero in every arm.  The global figure max|d| / max|ref| of tests/test_kernels_gpu.py is recorded next to it.

Bound, bf16 arms: err <= 3 * the rounding model's err on the same case.  rounding_model() below is plain torch in fp32 with the
roundings a flash kernel cannot avoid: P and dS rounded to bf16 before the second GEMM, outputs rounded to bf16; delta_from_O = True takes
delta = rowsum(dO * bf16(O)) as the one-kernel backward does, False recomputes rowsum(P * dP) (two-kernel form; the unfused path, which
also reads the STORED bf16 P in its softmax backward).  The factor 3 covers another summation order, the log2 domain and P kept
unnormalised until after the PV product.  tests/test_attention_model.py holds the model itself to absolute caps on the CPU, so that
3 x model cannot drift into a loose bound.
The one exception is a block whose reference is identically zero (N = 1: dQ = dK = 0, the block measured against dV's scale): there the
recompute model cancels to exactly 0, and the bound is 3 * (model + 2^-18).  2^-18 = 64 * 2^-24 is the one rounding the model cannot show
on its own: a 64-term fp32 dot product evaluated in two orders (MFMA dP against the fmaf chain of delta, exp2(s - lse) against 1).
Bound, fp32 arm: err <= 4 * max(e32, 2^-23), e32 = the same figure of the formula evaluated in plain fp32 torch on the CPU (measured
5e-7 .. 8e-7 per block on the sweep; the existing kind of bound: summation order and expf only).
The fused forward's log-sum-exp (fp32 [B, H, NKP] in `probs`, NKP = 16 * NKT) is compared too: |d| <= 1e-4 on unit-normal input, from
64-term fp32 accumulation of |s| <= 8 (64 * 2^-24 * 8 = 3e-5) plus v_exp_f32 / v_log_f32 at 1 ulp; a wrong NKP is off by O(1).

Contract (every run of every case): every buffer has the size include/rmcl.h prescribes (rmcl_attention_scratch_elems for probs, scores,
dS) between guard bytes - 256 in front, B * H * 256 * 4 + 4096 behind, more than the worst overrun of the N <= 8 sizing bug this file
found - which must be intact afterwards; out, dqkv and the scratch buffers start as NaN (a pad entry of lse / delta or a pad column of a score
row read without having been written shows as 0 * NaN) and out / dqkv hold none afterwards; qkv, dout and the mask are unchanged.

Measured figures, kernel next to model, go to the file named by RMCL_ATTN_PARITY_OUT when set (profiles/attention_parity.json is such a dump).
"""
import collections
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, stream, tdt  # noqa: E402

Case = collections.namedtuple("Case", "B N H mask family")
BLOCKS = ("out", "dQ", "dK", "dV")
E32 = 2.0 ** -18                    # 64-term fp32 dot product in two orders: added where the reference block is identically zero (docstring)
BF16_FACTOR, F32_FACTOR, F32_FLOOR = 3.0, 4.0, 2.0 ** -23
LSE_TOL = 1e-4
FAMILIES = ("normal", "qx4", "v+3", "k+2")
STRESS = FAMILIES[1:]
SWEEP_N = (1, 7, 8, 9, 16, 17, 63, 64, 65, 100, 127, 128, 129, 185, 191, 192, 193, 241, 255, 256)
ARM_N = (40, 100, 185, 241)         # one N per NKT arm
# arm -> (dtype, exact, `out` given to the backward, rmcl_tune_set key 2)
ARMS = {"fused_noout": (L.BF16, 0, False, 1), "fused_out": (L.BF16, 0, True, 1), "fused_key2_0": (L.BF16, 0, True, 0),
        "bf16_exact": (L.BF16, 1, False, 1), "f32_exact": (L.F32, 1, False, 1)}
TUNE_DEFAULTS = ((4, 8), (8, 256), (9, 1), (2, 1))
PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_ATTN_PARITY_OUT")
    if out and PARITY:
        # (allowed 0: the entry is exact in the model - N = 1: out, dV - and the assertion has held the kernel to 0 too)
        worst = max((v[0] / v[4] if v[4] else float(v[0] > 0) * 1e30, f"{case}:{arm}:{blk}")
                    for case, arms in PARITY.items() for arm, fig in arms.items() for blk, v in fig.items())
        with open(out, "w") as f:
            json.dump({"columns": ["kernel_worst_row", "model_worst_row", "kernel_global", "model_global", "allowed_worst_row"],
                       "model": "bf16 arms: rounding_model (one_kernel: delta_from_O); f32 arm: plain fp32 torch",
                       "largest_kernel_over_allowed": worst[0], "largest_at": worst[1], "cases": PARITY}, f, indent=1, sort_keys=True)


def nkp_of(N):
    """Rows of the fused kernels' per-(batch, head) statistics (include/rmcl.h)."""
    return 64 if N <= 64 else 128 if N <= 128 else 192 if N <= 192 else 256


def bf(x):
    return x.bfloat16().float()


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------ inputs, reference, model (CPU)
def make_mask(B, N, kind):
    m = torch.ones(B, N, dtype=torch.int32)
    if kind == "holes":                                    # the pattern of test_attention_fwd_bwd, clipped for tiny N
        m[0, max(N - 17, 0):max(N - 3, 0)] = 0
        if B > 1:
            m[1, min(5, N):min(9, N)] = 0
    elif kind == "tail":                                   # valid keys end inside a tile: whole trailing key tiles are masked
        m[0, {40: 20, 100: 50, 129: 100, 185: 100, 241: 150}.get(N, N // 2 + 1):] = 0
        if B > 1:
            m[1, N // 3 + 1:] = 0
    elif kind == "key0":                                   # one valid key
        m[0, 1:] = 0
    elif kind == "text":                                   # the real batch: text pad t..39, image-pad tail
        for b in range(B):
            m[b, (8, 39, 23)[b % 3]:40] = 0
            tail = min((13, 5, 0)[b % 3], N - 40)
            if tail > 0:
                m[b, N - tail:] = 0
    else:
        assert kind == "all"
    assert bool((m.sum(1) >= 1).all())                     # a fully masked sample is NaN in the reference too: out of scope
    return m


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fp32 qkv [B*N, 3D], dout [B*N, D] and the int32 mask [B, N] on the CPU."""
    B, N, H, kind, family = case
    D = H * 64
    g = torch.Generator(device="cpu").manual_seed(1)
    qkv = torch.randn(B * N, 3 * D, generator=g)
    g = torch.Generator(device="cpu").manual_seed(2)
    dout = torch.randn(B * N, D, generator=g)
    if family == "qx4":                                    # peaked softmax
        qkv[:, :D] *= 4
    elif family == "v+3":                                  # common offset in V: dP - delta is a difference of large numbers
        qkv[:, 2 * D:] += 3
    elif family == "k+2":
        qkv[:, D:2 * D] += 2
    else:
        assert family == "normal"
    return qkv, dout, make_mask(B, N, kind)


def kernel_values(case, dt):
    qkv, dout, mask = inputs(case)
    return (qkv, dout, mask) if dt == L.F32 else (bf(qkv), bf(dout), mask)


def split(out, dqkv, D):
    return {"out": out, "dQ": dqkv[:, :D], "dK": dqkv[:, D:2 * D], "dV": dqkv[:, 2 * D:]}


def attention_autograd(qkv, dout, mask, B, N, H, dtype):
    x = qkv.detach().to(dtype).clone().requires_grad_(True)
    t = x.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-2, -1)) * 0.125
    s = s.masked_fill(~mask.bool()[:, None, None, :], float("-inf"))
    o = (s.softmax(-1) @ t[2]).transpose(1, 2).reshape(B * N, H * 64)
    o.backward(dout.to(dtype))
    return split(o.detach(), x.grad, H * 64), torch.logsumexp(s.detach(), -1)


@functools.lru_cache(maxsize=None)
def reference(case, dt):
    """float64 blocks and log-sum-exp [B, H, N] on the values an arm of storage type dt reads."""
    B, N, H = case[:3]
    return attention_autograd(*kernel_values(case, dt), B, N, H, torch.float64)


def rounding_model(qkv, dout, mask, B, N, H, delta_from_O, stored_p=False):
    """The roundings a flash kernel cannot avoid, in plain fp32 torch (qkv / dout: bf16 values).  stored_p: the backward reads the bf16 P
    the forward stored (unfused path) instead of recomputing P in fp32."""
    t = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    do = dout.float().reshape(B, N, H, 64).transpose(1, 2)
    s = (q @ k.transpose(-2, -1)) * 0.125
    s = s.masked_fill(~mask.bool()[:, None, None, :], float("-inf"))
    p = s.softmax(-1)
    pb = bf(p)                                             # P -> bf16 before the PV and the P^T dO products
    o = bf(pb @ v)
    dp = do @ v.transpose(-2, -1)
    pg = pb if stored_p else p
    delta = (do * o).sum(-1, keepdim=True) if delta_from_O else (pg * dp).sum(-1, keepdim=True)
    ds = bf(pg * (dp - delta) * 0.125)                     # dS -> bf16 before the dS K and the dS^T Q products
    dq, dk, dv = bf(ds @ k), bf(ds.transpose(-2, -1) @ q), bf(pb.transpose(-2, -1) @ do)
    rows = lambda x: x.transpose(1, 2).reshape(B * N, H * 64)
    return {"out": rows(o), "dQ": rows(dq), "dK": rows(dk), "dV": rows(dv)}


def row_err(got, ref, fallback):
    got, ref = got.double(), ref.double()
    rn = ref.norm(dim=1)
    rms = float(rn.square().mean().sqrt()) or fallback
    return float(((got - ref).norm(dim=1) / rn.clamp_min(0.05 * rms)).max())


def glob_err(got, ref, fallback):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / (float(ref.abs().max()) or fallback))


def figures(got, ref):
    """{block: (worst-row error, global error)}; an identically zero reference block is measured against dV's scale."""
    rms_v = float(ref["dV"].double().norm(dim=1).square().mean().sqrt())
    max_v = float(ref["dV"].abs().max())
    return {b: (row_err(got[b], ref[b], rms_v), glob_err(got[b], ref[b], max_v)) for b in BLOCKS}


MODEL_KINDS = {"one_kernel": dict(delta_from_O=True), "two_kernel": dict(delta_from_O=False), "unfused": dict(delta_from_O=False, stored_p=True)}


@functools.lru_cache(maxsize=None)
def model_figures(case, kind):
    B, N, H = case[:3]
    if kind == "f32":
        return figures(attention_autograd(*kernel_values(case, L.F32), B, N, H, torch.float32)[0], reference(case, L.F32)[0])
    return figures(rounding_model(*kernel_values(case, L.BF16), B, N, H, **MODEL_KINDS[kind]), reference(case, L.BF16)[0])


def model_kind(case, arm):
    dt, exact, with_out, key2 = ARMS[arm]
    if dt == L.F32:
        return "f32"
    if exact or case.N > 256:
        return "unfused"
    return "one_kernel" if (with_out and key2 and case.N <= 192) else "two_kernel"


# ------------------------------------------------------------------------------------------ device side
class Guarded:
    """A device buffer of exactly `n` elements between guard bytes."""
    FRONT, BYTE = 256, 0xA5

    def __init__(self, n, dtype, back, fill):
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.FRONT + nbytes + back,), self.BYTE, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.FRONT:self.FRONT + nbytes].view(dtype)
        self.t.fill_(fill)
        self.nbytes = nbytes

    def intact(self):
        return bool((self.raw[:self.FRONT] == self.BYTE).all()) and bool((self.raw[self.FRONT + self.nbytes:] == self.BYTE).all())


def run_attention(case, dt, exact, with_out, expect_fail=False):
    """Forward + backward through the C ABI on guarded, exactly sized buffers; asserts the contract of the docstring and returns the
    results on the CPU (lse: the fused forward's log-sum-exp [B, H, N], else None)."""
    B, N, H = case[:3]
    D = H * 64
    qkv_c, dout_c, mask_c = kernel_values(case, dt)
    qkv, dout, mask = qkv_c.to(DEV, tdt(dt)), dout_c.to(DEV, tdt(dt)), mask_c.to(DEV)
    keep = (qkv.clone(), dout.clone(), mask.clone())
    ne = int(lib.rmcl_attention_scratch_elems(B, H, N))
    back = B * H * 256 * 4 + 4096
    nan = float("nan")
    buf = {"out": Guarded(B * N * D, tdt(dt), back, nan), "dqkv": Guarded(B * N * 3 * D, tdt(dt), back, nan),
           "probs": Guarded(ne, tdt(dt), back, nan), "scores": Guarded(ne, torch.float32, back, nan), "dS": Guarded(ne, tdt(dt), back, nan)}
    before = {n: b.raw.clone() for n, b in buf.items()} if expect_fail else None
    t = {n: b.t for n, b in buf.items()}
    rc_f = lib.rmcl_attention_fwd(P(qkv), P(mask), P(t["out"]), P(t["probs"]), P(t["scores"]), B, N, H, dt, exact, stream())
    rc_b = lib.rmcl_attention_bwd(P(qkv), P(mask), P(t["probs"]), P(dout), P(t["out"]) if with_out else None, P(t["dqkv"]), P(t["scores"]),
                                  P(t["dS"]), B, N, H, dt, exact, stream())
    torch.cuda.synchronize()
    for n, b in buf.items():
        assert b.intact(), f"{n}: guard bytes overwritten"
    assert torch.equal(bits(qkv), bits(keep[0])) and torch.equal(bits(dout), bits(keep[1])) and torch.equal(mask, keep[2])
    if expect_fail:
        assert rc_f != 0 and rc_b != 0, (rc_f, rc_b)
        for n, b in buf.items():
            assert torch.equal(b.raw, before[n]), f"{n} was written by a rejected call"
        return None
    check(rc_f, "attention_fwd")
    check(rc_b, "attention_bwd")
    out, dqkv = t["out"].view(B * N, D).cpu(), t["dqkv"].view(B * N, 3 * D).cpu()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dqkv).any())
    lse = None
    if dt == L.BF16 and not exact and N <= 256:
        nkp = nkp_of(N)
        lse = buf["probs"].raw[Guarded.FRONT:Guarded.FRONT + B * H * nkp * 4].view(torch.float32).view(B, H, nkp)[:, :, :N].cpu()
    res = split(out, dqkv, D)
    res["lse"] = lse
    res["probs"] = t["probs"]
    return res


def tuned(pairs):
    for k, v in pairs:
        check(lib.rmcl_tune_set(k, v))


def run_arm(case, arm):
    dt, exact, with_out, key2 = ARMS[arm]
    try:
        tuned([(2, key2)])
        return run_attention(case, dt, exact, with_out)
    finally:
        tuned([(2, 1)])


def same_bits(a, b, names=BLOCKS):
    return all(torch.equal(bits(a[n]), bits(b[n])) for n in names)


def assert_parity(case, arm, got, label=None):
    """Records and asserts the worst-row figures of one run against the model-derived bound; masked keys give exactly zero dK / dV."""
    dt = ARMS[arm][0]
    ref, lse_ref = reference(case, dt)
    kind = model_kind(case, arm)
    mod = model_figures(case, kind)
    fig = figures(got, ref)
    rec, bad = {}, []
    for b in BLOCKS:
        if dt == L.BF16:
            allowed = BF16_FACTOR * (mod[b][0] + (0.0 if bool(ref[b].any()) else E32))
        else:
            allowed = F32_FACTOR * max(mod[b][0], F32_FLOOR)
        rec[b] = [fig[b][0], mod[b][0], fig[b][1], mod[b][1], allowed]
        print(f"{tuple(case)} {arm} [{kind}] {b}: worst row {fig[b][0]:.3e} (model {mod[b][0]:.3e}, allowed {allowed:.3e})  "
              f"global {fig[b][1]:.3e} (model {mod[b][1]:.3e})")
        if not fig[b][0] <= allowed:
            bad.append((b, fig[b][0], allowed))
    PARITY.setdefault("B{}_N{}_H{}_{}_{}".format(*case), {})[label or arm] = rec
    masked = (inputs(case)[2].reshape(-1) == 0)
    for b in ("dK", "dV"):
        assert bool((got[b][masked] == 0).all()), f"{b}: rows of masked keys are not exactly zero"
    if got["lse"] is not None and case.family == "normal":
        dl = float((got["lse"].double() - lse_ref).abs().max())
        print(f"{tuple(case)} {arm} lse: max |d| {dl:.3e}")
        assert dl <= LSE_TOL, f"log-sum-exp off by {dl} (layout [B, H, NKP = {nkp_of(case.N)}])"
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 1. tile-count sweep
@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("N", SWEEP_N)
def test_tile_count_sweep(N, arm):
    """Unit-normal input, the hole mask, every N at which nkt_for or a launcher switches (64|65, 128|129, 192|193, 256) and the tiny N
    of the scratch-sizing fix; each arm run twice gives the same bits; with key 2 = 0, and with `out` given at N >= 193, the backward
    is the two-kernel one bit for bit."""
    case = Case(2, N, 12, "holes", "normal")
    got = run_arm(case, arm)
    assert_parity(case, arm, got)
    assert same_bits(got, run_arm(case, arm)), "run-to-run difference"
    if arm == "fused_key2_0" or (arm == "fused_out" and N >= 193):
        assert same_bits(got, run_arm(case, "fused_noout")), "not the two-kernel backward's bits"


# ------------------------------------------------------------------------------------------ 2. mask shapes
@pytest.mark.parametrize("arm", ["fused_noout", "fused_out", "f32_exact"])
@pytest.mark.parametrize("kind", ["tail", "key0", "text", "all"])
@pytest.mark.parametrize("N", ARM_N + (129,))
def test_mask_shapes(N, kind, arm):
    """Whole trailing key tiles masked (N = 129 with 100 valid, 241 with 150, ...), one valid key, the text-pad + image-pad pattern of a
    real batch, and no masked key at all."""
    case = Case(2, N, 12, kind, "normal")
    assert_parity(case, arm, run_arm(case, arm))


# ------------------------------------------------------------------------------------------ 3. stress inputs
@pytest.mark.parametrize("arm", ["fused_out", "fused_noout"])
@pytest.mark.parametrize("family", STRESS)
@pytest.mark.parametrize("N", ARM_N)
def test_stress_inputs(N, family, arm):
    """Peaked softmax (q x 4) and common offsets in V and K: where delta = rowsum(dO * bf16(O)) of the one-kernel backward costs
    precision (the model with delta_from_O says how much; N = 241 is two-kernel in both arms)."""
    case = Case(2, N, 12, "text", family)
    assert_parity(case, arm, run_arm(case, arm))


# ------------------------------------------------------------------------------------------ 4. head count
@pytest.mark.parametrize("arm", ["fused_out", "fused_noout"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("N", [100, 185])
def test_head_counts(N, H, arm):
    case = Case(2, N, H, "holes", "normal")
    assert_parity(case, arm, run_arm(case, arm))


# ------------------------------------------------------------------------------------------ 5. launch variants give the same bits
@pytest.mark.parametrize("N", [17, 100, 185, 256])
def test_forward_wave_counts_give_the_same_bits(N):
    case = Case(2, N, 12, "holes", "normal")
    try:
        res = {}
        for waves in (8, 4, 6, 12):
            tuned([(4, waves)])
            res[waves] = run_attention(case, L.BF16, 0, False)
    finally:
        tuned(TUNE_DEFAULTS)
    assert_parity(case, "fused_noout", res[8], label="fused_noout")
    for waves in (4, 6, 12):
        assert same_bits(res[waves], res[8], ("out", "lse")), waves


@pytest.mark.parametrize("N", [64, 100, 185])
def test_one_kernel_backward_variants_give_the_same_bits(N):
    """B = 3: 36 problems, which a persistent grid of 5 does not divide; 1, 2 or 3 key tiles per wave (3 only where it divides NKT)."""
    case = Case(3, N, 12, "text", "normal")
    try:
        tuned(TUNE_DEFAULTS)
        base = run_attention(case, L.BF16, 0, True)
        for tpw in (1, 2, 3):
            for wgs in (0, 5, 256):
                tuned([(9, tpw), (8, wgs)])
                assert same_bits(run_attention(case, L.BF16, 0, True), base), (tpw, wgs)
    finally:
        tuned(TUNE_DEFAULTS)
    assert_parity(case, "fused_out", base)


# ------------------------------------------------------------------------------------------ 6. above 256
@pytest.mark.parametrize("arm", ["fused_noout", "f32_exact"])
@pytest.mark.parametrize("N", [257, 281, 512])
def test_above_256_is_unfused(N, arm):
    """(bf16, exact = 0) leaves the fused kernels at N = 257 (281: max_image_len = -1 at 384 x 640; 512: the softmax kernels' limit)."""
    case = Case(1, N, 12, "holes", "normal")
    got = run_arm(case, arm)
    assert_parity(case, arm, got, label="bf16_fast_unfused" if arm == "fused_noout" else arm)
    if arm == "fused_noout":                               # `probs` holds probabilities [B, H, N, ldp], not a log-sum-exp
        assert got["lse"] is None
        row = got["probs"][:(N + 7) // 8 * 8].float().sum()
        assert abs(float(row) - 1.0) < 1e-2


@pytest.mark.parametrize("arm", ["fused_noout", "f32_exact"])
def test_n_513_is_rejected_before_anything_is_written(arm):
    dt, exact, with_out, _ = ARMS[arm]
    run_attention(Case(1, 513, 12, "holes", "normal"), dt, exact, with_out, expect_fail=True)
