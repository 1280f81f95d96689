"""-m gpu: the per-step kernels (PGD ascent step, AdamW, momentum update, queue write, patch cut, owner-side shard sum, LayerNorm with
a bf16 output) through the C ABI against plain torch float64 references of the same operation, at the sizes where their launchers take
another arm: fewer blocks than partial-maximum slots, one element group more than the capped grid covers in one pass, segment ends
on 64-element boundaries, the last legal queue slot, non-square images.

References are float64 on the values the kernel READS: lr, eps, betas, the momentum and the segment tables are rounded to fp32 first,
as the ABI does.  Tolerances.
  PGD step   elementwise 4 * 2^-24 * (|delta0| + lr |g| / den): the product, the quotient and the sum are one fp32 rounding each.
  AdamW      e32 = the deviation of the fp32 CPU oracle (oracle.rmcl_oracle.adamw_step) from the float64 formula, per tensor and step;
             allowed = 4 * max(e32, 2^-23 * max|ref|).
  EMA        elementwise 3 * 2^-24 * (|k| + |q|): two products and a sum.
  LayerNorm  bf16 storage: 2^-8 relative to the row scale (tests/test_kernels_gpu.py); mean and rstd within 1e-5 relative, row by row.
  everything else is a copy or a fixed-order fp32 sum and is compared bit for bit.
Measured deviations are collected in PARITY and written as JSON to the file named by RMCL_STEP_PARITY_OUT when that is set
(profiles/step_kernel_parity.json is such a dump)."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream, tdt  # noqa: E402
from oracle import rmcl_oracle as O  # noqa: E402

PARITY = {}
INF_BITS = 0x7F800000
ADAMW_FACTOR = 4.0


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_STEP_PARITY_OUT")
    if out and PARITY:
        with open(out, "w") as f:
            json.dump({"adamw_factor": ADAMW_FACTOR, "cases": PARITY}, f, indent=1, sort_keys=True)


def cpu_randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def f32(v):
    """The value an fp32 argument of the ABI carries, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, ref):
    """Bit equality of two tensors of one type; the comparison runs where `got` lives."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    return torch.equal(bits(got), bits(ref.to(got.device)))


def rejected(rc, word):
    assert rc == -1, rc
    assert word.encode() in lib.rmcl_last_error(), lib.rmcl_last_error()


# ------------------------------------------------------------------------------------------ 1. PGD step
PGD_B = 3
PGD_PER = [4, 1028, 3072, 3 * 3072, 64 * 1024 - 4, 64 * 1024 + 4, 144 * 3072]
PGD_LR, PGD_EPS = 0.01, 0.005


@functools.lru_cache(maxsize=None)
def pgd_inputs(per, dt):
    """g [3, per] in the gradient type (CPU), delta0 [3, per] f32.  Sample 0 has its largest |g| in its LAST four elements, sample 1
    in its FIRST four (a skipped tail or head changes the denominator), sample 2 is all zero (the 1e-8 floor: delta unchanged).
    The planted maximum is the row's own maximum + 0.5, so the step keeps the size it has on a real gradient."""
    g = cpu_randn(PGD_B, per, seed=per % 9973 + 1)
    signs = torch.tensor([1.0, -1.0, -1.0, 1.0])
    g[0, -4:] = (g[0].abs().max() + 0.5) * signs
    g[1, :4] = -(g[1].abs().max() + 0.5) * signs
    g[2] = 0
    g = g.to(tdt(dt))
    delta0 = (cpu_randn(PGD_B, per, seed=per % 9973 + 2) * 0.002).clamp(-PGD_EPS, PGD_EPS)
    return g, delta0


def pgd_reference(g, delta0, lr, eps):
    """float64 clamp(delta0 + lr g / max(max|g_b|, 1e-8)) and the elementwise allowance."""
    lr, eps, g64, d64 = f32(lr), f32(eps), g.double(), delta0.double()
    den = g64.abs().amax(dim=1, keepdim=True).clamp_min(f32(1e-8))
    step = lr * g64 / den
    ref = d64 + step
    if eps > 0:
        ref = ref.clamp(-eps, eps)
    return ref, 4 * 2.0 ** -24 * (d64.abs() + step.abs()), eps


def pgd_scratch():
    return torch.full((64 * PGD_B,), INF_BITS, dtype=torch.int32, device=DEV)


def pgd_blocks(per):
    return min((per + 1023) // 1024, 64)


def assert_pgd_scratch(amax, per):
    """Slots at or beyond the launch's block count were neither written ..."""
    a = amax.cpu().view(PGD_B, 64)
    nb = pgd_blocks(per)
    assert (a[:, nb:] == INF_BITS).all()
    assert (a[:, :nb] != INF_BITS).all()


def assert_pgd_delta(got, g, delta0, lr, eps, what):
    """... nor read: a denominator of +inf would leave delta0 where it was."""
    ref, allowed, eps32 = pgd_reference(g, delta0, lr, eps)
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    ratio = float(((got - ref).abs() / allowed.clamp_min(1e-300)).max())
    fig = {"max_dev": float((got - ref).abs().max()), "max_dev_over_allowed": ratio}
    if eps32 > 0:
        hi, lo = ref == eps32, ref == -eps32
        fig.update(frac_inside=float((ref.abs() < eps32).double().mean()), frac_hi=float(hi.double().mean()), frac_lo=float(lo.double().mean()))
    print(what, fig)
    PARITY[what] = fig
    assert ((got - ref).abs() <= allowed).all(), (what, fig)
    if eps32 > 0:
        assert (got[hi] == eps32).all() and (got[lo] == -eps32).all(), what
        assert float(got.abs().max()) <= eps32
    assert torch.equal(got[2], delta0[2].double())                              # all-zero gradient: nothing moves
    return fig


@pytest.mark.parametrize("dt", [L.F32, L.BF16])
@pytest.mark.parametrize("per", PGD_PER)
def test_pgd_step_against_fp64(per, dt):
    g, delta0 = pgd_inputs(per, dt)
    ref, _, eps32 = pgd_reference(g, delta0, PGD_LR, PGD_EPS)
    if per >= 3072:                                                              # the input exercises the clamp AND leaves most elements inside it
        assert float((ref.abs() < eps32).double().mean()) >= 0.5
        assert float((ref == eps32).double().mean()) >= 0.02 and float((ref == -eps32).double().mean()) >= 0.02
    gd, delta, amax = g.to(DEV), delta0.to(DEV), pgd_scratch()
    check(lib.rmcl_pgd_step(P(gd), dt, P(delta), P(amax), PGD_B, I64(per), F(PGD_LR), F(PGD_EPS), stream()), "pgd_step")
    assert_pgd_delta(delta, g, delta0, PGD_LR, PGD_EPS, f"pgd/{per}/{'bf16' if dt else 'f32'}")
    assert_pgd_scratch(amax, per)


@pytest.mark.parametrize("dt", [L.F32, L.BF16])
@pytest.mark.parametrize("per", [1028, 64 * 1024 + 4])
def test_pgd_step_without_clamp(per, dt):
    """eps = 0: no clamp, every element is informative."""
    g, delta0 = pgd_inputs(per, dt)
    gd, delta, amax = g.to(DEV), delta0.to(DEV), pgd_scratch()
    check(lib.rmcl_pgd_step(P(gd), dt, P(delta), P(amax), PGD_B, I64(per), F(PGD_LR), F(0.0), stream()), "pgd_step")
    assert_pgd_delta(delta, g, delta0, PGD_LR, 0.0, f"pgd_noclamp/{per}/{'bf16' if dt else 'f32'}")
    assert float(delta.abs().max()) > PGD_EPS                                    # (it really was not clamped)
    delta2, out = delta0.to(DEV), torch.empty(PGD_B, per, device=DEV)
    base = cpu_randn(PGD_B, per, seed=5).to(DEV)
    check(lib.rmcl_pgd_step_fused(P(gd), dt, P(delta2), P(pgd_scratch()), PGD_B, I64(per), F(PGD_LR), F(0.0), P(base), P(out), L.F32, 0,
                                  stream()), "pgd_step_fused")
    assert torch.equal(delta2, delta) and torch.equal(out, base + delta)


@pytest.mark.parametrize("dt,odt", [(L.BF16, L.BF16), (L.F32, L.F32), (L.F32, L.BF16)])
@pytest.mark.parametrize("per", PGD_PER)
def test_pgd_step_fused_bitwise(per, dt, odt):
    """rmcl_pgd_step_fused = rmcl_pgd_step + the operand the loop forms next, bit for bit (test_pgd_step_fused of
    tests/test_kernels_gpu.py) at every grid shape, each call with its own +inf-filled scratch."""
    g, delta0 = pgd_inputs(per, dt)
    gd, d0 = g.to(DEV), delta0.to(DEV)
    base = cpu_randn(PGD_B, per, seed=per % 9973 + 3).to(DEV)
    ref = d0.clone()
    check(lib.rmcl_pgd_step(P(gd), dt, P(ref), P(pgd_scratch()), PGD_B, I64(per), F(PGD_LR), F(PGD_EPS), stream()), "pgd_step")
    want0 = torch.zeros_like(d0)
    check(lib.rmcl_pgd_step(P(gd), dt, P(want0), P(pgd_scratch()), PGD_B, I64(per), F(PGD_LR), F(PGD_EPS), stream()), "pgd_step")
    for flags in (0, L.PGD_SUM_PREV, L.PGD_DELTA_ZERO, L.PGD_DELTA_ZERO | L.PGD_SUM_PREV):
        zero = bool(flags & L.PGD_DELTA_ZERO)
        delta = torch.full_like(d0, float("nan")) if zero else d0.clone()        # (DELTA_ZERO must not read the buffer)
        out = torch.empty(PGD_B, per, dtype=tdt(odt), device=DEV)
        amax = pgd_scratch()
        check(lib.rmcl_pgd_step_fused(P(gd), dt, P(delta), P(amax), PGD_B, I64(per), F(PGD_LR), F(PGD_EPS), P(base), P(out), odt, flags,
                                      stream()), "pgd_step_fused")
        want, old = (want0, torch.zeros_like(d0)) if zero else (ref, d0)
        assert torch.equal(delta, want), flags
        op = (base + old) + want if (flags & L.PGD_SUM_PREV) and not zero else base + want
        assert same_bits(out, op.to(tdt(odt))), flags
        assert_pgd_scratch(amax, per)
    delta = d0.clone()                                                           # no operand: the update alone
    check(lib.rmcl_pgd_step_fused(P(gd), dt, P(delta), P(pgd_scratch()), PGD_B, I64(per), F(PGD_LR), F(PGD_EPS), None, None, odt, 0,
                                  stream()), "pgd_step_fused")
    assert torch.equal(delta, ref)


def test_pgd_step_rejects_per_sample_not_a_multiple_of_4():
    g, delta, amax = torch.zeros(PGD_B, 8, device=DEV), torch.ones(PGD_B, 8, device=DEV), pgd_scratch()
    rejected(lib.rmcl_pgd_step(P(g), L.F32, P(delta), P(amax), PGD_B, I64(6), F(PGD_LR), F(PGD_EPS), stream()), "per_sample")
    rejected(lib.rmcl_pgd_step_fused(P(g), L.F32, P(delta), P(amax), PGD_B, I64(6), F(PGD_LR), F(PGD_EPS), None, None, L.F32, 0, stream()),
             "per_sample")
    torch.cuda.synchronize()
    assert (delta == 1).all() and (amax == INF_BITS).all()


# ------------------------------------------------------------------------------------------ 2. AdamW
BIG_4096 = 4096 * 1024 + 1028       # one pass of the 4096-block grid covers 4096 * 1024 elements: the grid-stride loop iterates
ADAMW_MULT = [1.0, 10.0, 0.1, 5.0, 0.0]
ADAMW_WD = [0.01, 0.0, 0.1, 0.0, 0.01]
# multiples of 64, none of 1024; [0, 64) is a segment of exactly 64 elements.  The fourth end lies 192 elements INSIDE the second pass of
# the grid-stride loop: that pass looks up a segment with a non-zero multiplier (5), crosses a boundary and then meets lr_mult = 0
ADAMW_ENDS = [64, 192, 4160, 4096 * 1024 + 192]
ADAMW_STEPS = [1, 2, 3, 10000]


def adamw_segments(n, nseg):
    """Exclusive segment ends.  nseg = 5 on a short arena leaves EMPTY trailing segments (end == previous end): the lookup must never
    land in one."""
    return [n] if nseg == 1 else [min(e, n) for e in ADAMW_ENDS] + [n]


@pytest.mark.parametrize("nseg", [1, 5])
@pytest.mark.parametrize("n", [64, 4160, BIG_4096])
def test_adamw_against_fp64(n, nseg):
    """m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps); p -= lr wd p with
    g = grad * grad_scale (csrc/embed_misc.hip), steps 1, 2, 3 on one state and then step 10000 (both bias corrections ~ 1).  Run with
    and without the bf16 shadow: p, m, v must not depend on it and the shadow is bf16(p) of the kernel's own p, bit for bit (round to
    nearest even, lane order of the packed pairs)."""
    ends = adamw_segments(n, nseg)
    mult32, wd32 = [f32(x) for x in ADAMW_MULT[:nseg]], [f32(x) for x in ADAMW_WD[:nseg]]
    lr, b1, b2, eps, gs = f32(1e-3), f32(0.9), f32(0.98), f32(1e-8), f32(1.0 / 3.0)
    p0, g = cpu_randn(n, seed=n % 977 + 1), cpu_randn(n, seed=n % 977 + 2)
    starts = [0] + ends[:-1]
    seg_of = torch.bucketize(torch.arange(n), torch.tensor(ends), right=True)   # first segment with end > e
    assert int(seg_of.max()) < nseg
    mult_e, wd_e = torch.tensor(mult32, dtype=torch.float64)[seg_of], torch.tensor(wd32, dtype=torch.float64)[seg_of]
    p64, m64, v64, g64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), g.double() * gs
    p32, m32, v32, g32 = p0.clone(), torch.zeros(n), torch.zeros(n), g * torch.tensor(gs)
    dev = {lp: [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] for lp in (True, False)}
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    gd = g.to(DEV)
    seg_end = torch.tensor(ends, dtype=torch.int64, device=DEV)
    mult_d, wd_d = torch.tensor(mult32, device=DEV), torch.tensor(wd32, device=DEV)
    edges = sorted({e for e in ends if e < n})
    for step in ADAMW_STEPS:
        m64 = b1 * m64 + (1 - b1) * g64
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        p64 = p64 - (lr * mult_e) * (1 - b2 ** step) ** 0.5 / (1 - b1 ** step) * m64 / (v64.sqrt() + eps)
        p64 = torch.where(wd_e > 0, p64 - (lr * mult_e) * wd_e * p64, p64)
        for s, e, mu, w in zip(starts, ends, mult32, wd32):
            O.adamw_step(p32[s:e], g32[s:e], m32[s:e], v32[s:e], step, lr * mu, w, b1, b2, eps)
        for lp in (True, False):
            p, m, v = dev[lp]
            check(lib.rmcl_adamw_f32(P(p), P(gd), P(m), P(v), P(shadow if lp else None), P(seg_end), P(mult_d), P(wd_d), nseg, F(lr), F(b1),
                                     F(b2), F(eps), step, F(gs), I64(n), stream()), "adamw")
        for a, b in zip(dev[True], dev[False]):
            assert torch.equal(a, b), step
        assert same_bits(shadow, dev[True][0].to(torch.bfloat16)), step
        for name, got, ref, twin in (("p", dev[True][0], p64, p32), ("m", dev[True][1], m64, m32), ("v", dev[True][2], v64, v32)):
            got = got.double().cpu()
            assert torch.isfinite(got).all()
            e32 = float((twin.double() - ref).abs().max())
            allowed = ADAMW_FACTOR * max(e32, 2.0 ** -23 * float(ref.abs().max()))
            err = (got - ref).abs()
            fig = {"e32": e32, "kernel_dev": float(err.max()), "allowed": allowed, "ratio": float(err.max()) / allowed}
            print(f"adamw n={n} nseg={nseg} step={step} {name}", fig)
            PARITY[f"adamw/{n}/{nseg}/step{step}/{name}"] = fig
            for edge in edges:                                                   # an off-by-one segment changes these by a factor
                lo, hi = float(err[edge - 64:edge].max()), float(err[edge:edge + 64].max())
                assert lo <= allowed, f"{name}: the 64 elements BELOW the segment end {edge}: {lo} > {allowed} (step {step})"
                assert hi <= allowed, f"{name}: the 64 elements FROM the segment end {edge} on: {hi} > {allowed} (step {step})"
            assert float(err.max()) <= allowed, (name, step, fig)
    if nseg == 5:                                                                # lr_mult = 0: the last segment's weights never move
        s = ends[-2]
        assert torch.equal(dev[True][0][s:].cpu(), p0[s:])


# ------------------------------------------------------------------------------------------ 3. momentum update
@pytest.mark.parametrize("with_lp", [True, False])
@pytest.mark.parametrize("m", [0.999, 0.0, 1.0])
@pytest.mark.parametrize("n", [4, 1028, BIG_4096])
def test_ema_against_fp64(n, m, with_lp):
    k0, q = cpu_randn(n, seed=n % 977 + 11), cpu_randn(n, seed=n % 977 + 12)
    k, qd = k0.to(DEV), q.to(DEV)
    lp = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if with_lp else None
    check(lib.rmcl_ema_f32(P(k), P(qd), P(lp), F(m), I64(n), stream()), "ema")
    m32 = f32(m)
    ref = k0.double() * m32 + q.double() * (1.0 - m32)                           # (1 - m is exact in fp32 for m in [0.5, 1] and for m = 0)
    err = (k.double().cpu() - ref).abs()
    allowed = 3 * 2.0 ** -24 * (k0.double().abs() + q.double().abs())
    PARITY[f"ema/{n}/{m}/{int(with_lp)}"] = {"max_dev": float(err.max()), "max_dev_over_allowed": float((err / allowed).max())}
    assert (err <= allowed).all(), float((err / allowed).max())
    if m == 1.0:
        assert same_bits(k, k0)
    if m == 0.0:
        assert same_bits(k, q)
    if with_lp:
        assert same_bits(lp, k.to(torch.bfloat16))
    assert torch.equal(qd.cpu(), q)


# ------------------------------------------------------------------------------------------ 4. queue write
@pytest.mark.parametrize("n,ptr,Kq", [(8, 1024 - 8, 1024), (3, 0, 1024), (70, 1024 - 70, 1024), (64, 65536 - 64, 65536)])
def test_enqueue_bitwise(n, ptr, Kq):
    proj = 128
    queue0, keys = cpu_randn(proj, Kq, seed=21), cpu_randn(n, proj, seed=22)
    queue, keysd = queue0.to(DEV), keys.to(DEV)
    check(lib.rmcl_enqueue_f32(P(queue), P(keysd), n, proj, I64(Kq), I64(ptr), stream()), "enqueue")
    ref = queue0.clone()
    ref[:, ptr:ptr + n] = keys.t()
    assert same_bits(queue, ref)
    rejected(lib.rmcl_enqueue_f32(P(queue), P(keysd), n, proj, I64(Kq), I64(-1), stream()), "enqueue")
    rejected(lib.rmcl_enqueue_f32(P(queue), P(keysd), n, proj, I64(Kq), I64(Kq + 1 - n), stream()), "enqueue")
    torch.cuda.synchronize()
    assert same_bits(queue, ref)


# ------------------------------------------------------------------------------------------ 5. patch cut
@pytest.mark.parametrize("shape", [(3, 3, 64, 96, 32), (2, 3, 96, 32, 32), (1, 1, 8, 12, 4), (2, 3, 384, 384, 32)])
def test_im2patch_and_inverse_bitwise(shape):
    """Both directions against the permutation itself, each from its own random input (no round trip: a consistently wrong pair of
    directions passes one)."""
    B, Cc, H, W, ps = shape
    gh, gw = H // ps, W // ps
    img = cpu_randn(B, Cc, H, W, seed=31)
    imgd = img.to(DEV)
    pat = torch.full((B * gh * gw, Cc * ps * ps), float("nan"), device=DEV)
    check(lib.rmcl_im2patch_f32(P(imgd), P(pat), B, Cc, H, W, ps, 0, stream()), "im2patch")
    ref = img.reshape(B, Cc, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, Cc * ps * ps)
    assert same_bits(pat, ref)
    rows = cpu_randn(B * gh * gw, Cc * ps * ps, seed=32)
    rowsd = rows.to(DEV)
    back = torch.full((B, Cc, H, W), float("nan"), device=DEV)
    check(lib.rmcl_im2patch_f32(P(back), P(rowsd), B, Cc, H, W, ps, 1, stream()), "patch2im")
    ref_img = rows.reshape(B, gh, gw, Cc, ps, ps).permute(0, 3, 1, 4, 2, 5).reshape(B, Cc, H, W)
    assert same_bits(back, ref_img)
    assert torch.equal(rowsd.cpu(), rows) and torch.equal(imgd.cpu(), img)


def test_im2patch_rejects_a_side_that_is_no_multiple_of_the_patch():
    img, pat = torch.zeros(1, 3, 64, 64, device=DEV), torch.ones(4, 3072, device=DEV)
    rejected(lib.rmcl_im2patch_f32(P(img), P(pat), 1, 3, 40, 64, 32, 0, stream()), "im2patch")
    rejected(lib.rmcl_im2patch_f32(P(img), P(pat), 1, 3, 64, 40, 32, 1, stream()), "im2patch")
    torch.cuda.synchronize()
    assert (pat == 1).all() and (img == 0).all()


# ------------------------------------------------------------------------------------------ 6. shard sum
BIG_8192 = 8192 * 1024 + 1028       # one pass of the 8192-block grid covers 8192 * 1024 elements


@functools.lru_cache(maxsize=None)
def shard_base(n):
    return cpu_randn(n, seed=41)


@pytest.mark.parametrize("wire", ["f32", "bf16"])
@pytest.mark.parametrize("n", [4, 1028, BIG_8192])
@pytest.mark.parametrize("W", [1, 3])
def test_shard_sum_outputs_each_on_its_own(W, n, wire):
    base = shard_base(n).to(DEV)
    pieces = torch.stack([base, base.flip(0) * 0.37, base.roll(1) * 3.0][:W]).contiguous()
    dt = L.BF16 if wire == "bf16" else L.F32
    pieces = pieces.to(tdt(dt))
    want = pieces[0].float().clone()                                             # rank order, fp32 accumulation
    for w in range(1, W):
        want += pieces[w].float()
    keep = pieces.clone()

    def run(with32, withw):
        out32, outw = torch.full((n,), -3.0, device=DEV), torch.full((n,), -3.0, dtype=tdt(dt), device=DEV)
        check(lib.rmcl_shard_sum(P(pieces), dt, W, I64(n), P(out32 if with32 else None), P(outw if withw else None), stream()), "shard_sum")
        assert same_bits(out32, want if with32 else torch.full_like(want, -3.0))
        assert same_bits(outw, want.to(tdt(dt)) if withw else torch.full_like(outw, -3.0))

    run(True, True)
    run(True, False)
    run(False, True)
    assert same_bits(pieces, keep)


# ------------------------------------------------------------------------------------------ 7. LayerNorm, bf16 output
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("MD", [(1, 768), (203, 768), (37, 512), (5, 4)])
def test_layernorm_fwd_bf16_output(MD, relu):
    (M, D), eps = MD, 1e-6
    x = cpu_randn(M, D, seed=51 + M) * 2 + 1.5
    w, b = 1 + 0.1 * cpu_randn(D, seed=52), 0.1 * cpu_randn(D, seed=53)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = torch.zeros(M, D, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.full((M,), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    check(lib.rmcl_layernorm_fwd(P(xd), P(wd), P(bd), F(eps), P(y), L.BF16, P(mean), P(rstd), M, D, relu, stream()), "layernorm_fwd")
    x64 = x.double()
    mu, var = x64.mean(1), x64.var(1, unbiased=False)
    rs = (var + f32(eps)).rsqrt()
    ref = (x64 - mu[:, None]) * rs[:, None] * w.double() + b.double()
    scale = ref.abs().amax(1)                                                    # the row scale BEFORE the ReLU
    if relu:
        ref = ref.clamp_min(0)
    yk = y.double().cpu()
    assert torch.isfinite(yk).all()
    err = (yk - ref).abs().amax(1)
    PARITY[f"layernorm_bf16/{M}x{D}/relu{relu}"] = {"max_dev_over_row_scale": float((err / scale).max()), "allowed": 2.0 ** -8}
    assert (err <= 2.0 ** -8 * scale).all(), float((err / scale).max())
    mean_rel, rstd_rel = (mean.double().cpu() - mu).abs() / mu.abs(), (rstd.double().cpu() - rs).abs() / rs
    PARITY[f"layernorm_bf16/{M}x{D}/relu{relu}"].update(mean_rel=float(mean_rel.max()), rstd_rel=float(rstd_rel.max()), stat_allowed=1e-5)
    assert (mean_rel <= 1e-5).all(), float(mean_rel.max())
    assert (rstd_rel <= 1e-5).all(), float(rstd_rel.max())
    y32 = torch.zeros(M, D, device=DEV)                                          # the fp32 output of the same call rounds to the same bits
    check(lib.rmcl_layernorm_fwd(P(xd), P(wd), P(bd), F(eps), P(y32), L.F32, P(mean), P(rstd), M, D, relu, stream()), "layernorm_fwd")
    assert same_bits(y, y32.to(torch.bfloat16))
