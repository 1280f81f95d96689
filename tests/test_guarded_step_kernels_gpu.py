"""-m gpu: the guarded optimizer step's kernels through the C ABI against float64 references on the host (csrc/optim.hip).

rmcl_grad_stats_f32   one pass over the gradient: the non-finite count is exact; the sum of squares of the finite elements is compared
                      with math.fsum of the exact squares (the square of an fp32 is exact in a double and every term is positive, so
                      ANY summation order stays within n * 2^-53 relative); norm and clip_coef within 4 * 2^-24 relative of the float64
                      formula (+ one fp32 denormal step, 2^-149, absolute: below 2^-126 an fp32 carries fewer than 24 bits); the same
                      bytes of ctl and workspace on a second call; guard bytes around both untouched.
                      clip_coef = min(1, max_norm / (norm + 1e-6)) is torch's clip_grad_norm_: it is exactly 1 for max_norm = 0 (off) and
                      for max_norm >= norm + 1e-6.  The cases use max_norm = 0, norm / 2 (must clip) and 2 norm + 2e-6 (must not).
rmcl_adamw_guarded_f32  the sizes, segment tables, steps and tolerance rule of tests/test_step_kernels_gpu.py test_adamw_against_fp64
                      (allowed = 4 * max(e32, 2^-23 * max|ref|) per tensor, e32 = the fp32 CPU oracle's own deviation from float64):
                      (a) unclipped, m and v bit-equal to rmcl_adamw_f32; (b) a skipped step writes nothing and the next clean step is step
                      applied + 1; (c) clipping; (d) rejected calls.
Measured figures go to the file named by RMCL_GUARDED_PARITY_OUT when set (profiles/guarded_step_parity.json is such a dump)."""
import ctypes as C
import functools
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream  # noqa: E402
from oracle import rmcl_oracle as O  # noqa: E402

PARITY = {}
ADAMW_FACTOR = 4.0
GUARD = 256
SENTINEL = 0xA5
CTL_BYTES = C.sizeof(L.StepCtl)
STATS_BLOCKS = 1024                         # csrc/optim.hip RMCL_STATS_MAX_BLOCKS; a block covers 1024 elements per pass
PARTIAL = 3 * 1024 + 516                    # four blocks, the last one with 129 of its 256 threads at work
BIG_1024 = STATS_BLOCKS * 1024 + 1028       # one pass of the capped grid covers 1024 * 1024 elements: the grid-stride loop iterates
BIG_UNROLL = 4 * STATS_BLOCKS * 1024 + 1028 # the first 257 threads take the four-loads-in-flight body once, the rest the plain loop
STATS_SIZES = [4, 64, 4160, PARTIAL, BIG_1024]
B1, B2 = 0.9, 0.98


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_GUARDED_PARITY_OUT")
    if out and PARITY:
        with open(out, "w") as f:
            json.dump({"adamw_factor": ADAMW_FACTOR, "cases": PARITY}, f, indent=1, sort_keys=True)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def cpu_randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    return torch.equal(bits(got), bits(ref.to(got.device)))


def rejected(rc, word):
    assert rc == -1, rc
    assert word.encode() in lib.rmcl_last_error(), lib.rmcl_last_error()


def fenced(nbytes):
    """(whole buffer, the nbytes in its middle): GUARD sentinel bytes on either side."""
    buf = torch.full((2 * GUARD + nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def fences_intact(buf, nbytes):
    b = buf.cpu()
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + nbytes:] == SENTINEL).all())


def ws_bytes(n):
    return int(lib.rmcl_grad_stats_ws_bytes(I64(n)))


def new_ctl(**fields):
    buf, ctl = fenced(CTL_BYTES)
    ctl.copy_(L.StepCtl(**fields).to_tensor(DEV))
    return buf, ctl


def run_stats(gd, gs, max_norm, ws, ctl):
    check(lib.rmcl_grad_stats_f32(P(gd), I64(gd.numel()), F(gs), F(max_norm), F(B1), F(B2), P(ws), P(ctl), stream()), "grad_stats")
    return L.StepCtl.from_tensor(ctl)


def bias_corrections(step):
    b1, b2 = f32(B1), f32(B2)
    return f32(1.0 - b1 ** step), f32(math.sqrt(1.0 - b2 ** step))


# ------------------------------------------------------------------------------------------ 1. statistics
@functools.lru_cache(maxsize=None)
def stats_input(n, kind):
    if kind == "zeros":
        return torch.zeros(n)
    if kind == "denormal":                                                       # every element a non-zero fp32 denormal, either sign
        gen = torch.Generator(device="cpu").manual_seed(n % 977 + 5)
        mant = torch.randint(1, 1 << 23, (n,), generator=gen, dtype=torch.int32)
        sign = torch.randint(0, 2, (n,), generator=gen, dtype=torch.int32) * (-(1 << 31))
        x = (mant | sign).view(torch.float32)
        assert float(x.abs().max()) < 2.0 ** -126 and float(x.abs().min()) > 0
        return x
    return cpu_randn(n, seed=n % 977 + 3, scale=float(kind))


@functools.lru_cache(maxsize=None)
def exact_sumsq(n, kind):
    x = stats_input(n, kind).double()
    return math.fsum((x * x).tolist())


def check_decision(c, ref_sumsq, n, gs, max_norm, what):
    """sumsq, norm and clip_coef of one statistics call against float64."""
    assert abs(c.sumsq - ref_sumsq) <= n * 2.0 ** -53 * ref_sumsq, (what, c.sumsq, ref_sumsq)
    norm_ref = f32(gs) * math.sqrt(ref_sumsq)
    tol = lambda ref: 4 * 2.0 ** -24 * abs(ref) + 2.0 ** -149
    assert abs(c.norm - norm_ref) <= tol(norm_ref), (what, c.norm, norm_ref)
    mx = f32(max_norm)
    coef_ref = min(1.0, mx / (norm_ref + f32(1e-6))) if mx > 0 else 1.0
    assert abs(c.clip_coef - coef_ref) <= tol(coef_ref), (what, c.clip_coef, coef_ref)
    fig = {"sumsq_rel": abs(c.sumsq - ref_sumsq) / ref_sumsq if ref_sumsq else 0.0, "sumsq_allowed_rel": n * 2.0 ** -53,
           "norm_rel": abs(c.norm - norm_ref) / norm_ref if norm_ref else 0.0, "coef_rel": abs(c.clip_coef - coef_ref) / coef_ref}
    PARITY[what] = fig
    return norm_ref


# every input at the five sizes; the unrolled body of the largest size on the two inputs whose sums differ most
STATS_CASES = [(n, kind) for n in STATS_SIZES for kind in ("1e-3", "1", "1e20", "denormal", "zeros")] + [(BIG_UNROLL, "1"), (BIG_UNROLL, "1e20")]


@pytest.mark.parametrize("n,kind", STATS_CASES)
def test_grad_stats_against_fp64(n, kind):
    x, ref = stats_input(n, kind), exact_sumsq(n, kind)
    if kind == "1e20":
        assert not math.isfinite(float((x * x).sum()))                            # an fp32 sum of squares overflows on this FINITE input
    gd, gs = x.to(DEV), 1.0 / 3.0
    nws = ws_bytes(n)
    assert nws == 16 * min((n // 4 + 255) // 256, STATS_BLOCKS)
    norm_ref = f32(gs) * math.sqrt(ref)
    for max_norm in (0.0, 0.5 * norm_ref, 2.0 * norm_ref + 2e-6):
        wbuf, ws = fenced(nws)
        cbuf, ctl = new_ctl(applied=2, skipped=5)
        c = run_stats(gd, gs, max_norm, ws, ctl)
        what = f"stats/{n}/{kind}/max_norm{max_norm:.3g}"
        check_decision(c, ref, n, gs, max_norm, what)
        assert c.nonfinite == 0 and c.skip == 0, what
        assert (c.applied, c.skipped) == (3, 5), what
        assert (c.bc1, c.bc2s) == bias_corrections(3), what
        mx = f32(max_norm)
        assert (c.clip_coef == 1.0) == (mx == 0 or mx >= c.norm + f32(1e-6)), (what, c.clip_coef, mx, c.norm)
        if mx > 0:
            assert (c.clip_coef < 1.0) == (mx < c.norm), what
        print(what, PARITY[what], "norm", c.norm, "coef", c.clip_coef)
        first = (cbuf.cpu().clone(), wbuf.cpu().clone())
        wbuf2, ws2 = fenced(nws)
        cbuf2, ctl2 = new_ctl(applied=2, skipped=5)
        run_stats(gd, gs, max_norm, ws2, ctl2)
        assert torch.equal(cbuf2.cpu(), first[0]) and torch.equal(wbuf2.cpu(), first[1]), what       # identical bytes on every call
        assert fences_intact(wbuf, nws) and fences_intact(cbuf, CTL_BYTES), what
        assert not bool((ws.cpu() == SENTINEL).all())                            # (the workspace WAS written)
    assert torch.equal(gd.cpu(), x)


def poison_positions(n):
    pos = {"first": 0, "last": n - 1}
    if n > 2048:
        pos.update(block_first=1024, block_last=1023)
    if n == 4160:
        pos["tail"] = 4096 + 30                                                  # the fifth block holds 64 elements
    if n == PARTIAL:
        pos["tail"] = 3 * 1024 + 300
    if n >= BIG_1024:
        pos["tail"] = n - 500                                                    # reached in a later pass of the grid-stride loop
        pos["second_pass_first"] = STATS_BLOCKS * 1024
    return pos


@pytest.mark.parametrize("n", STATS_SIZES + [BIG_UNROLL])
def test_grad_stats_counts_every_nonfinite_element(n):
    x = stats_input(n, "1").clone()
    gd, gs = x.to(DEV), 0.5
    nws = ws_bytes(n)
    pos = poison_positions(n)
    sq = (x.double() * x.double())
    total = exact_sumsq(n, "1")
    for where, i in pos.items():
        for bad in (float("nan"), float("inf"), float("-inf")):
            keep = float(x[i])
            gd[i] = bad
            wbuf, ws = fenced(nws)
            cbuf, ctl = new_ctl(applied=7, skipped=1, bc1=0.25, bc2s=0.5)
            c = run_stats(gd, gs, 1.0, ws, ctl)
            gd[i] = keep
            what = f"stats_poison/{n}/{where}/{bad}"
            assert c.nonfinite == 1 and c.skip == 1, (what, c.nonfinite, c.skip)
            assert (c.applied, c.skipped, c.bc1, c.bc2s) == (7, 2, 0.25, 0.5), what   # a dropped step leaves the step number alone
            rest = total - float(sq[i])                                              # the FINITE elements still add up
            assert abs(c.sumsq - rest) <= (n * 2.0 ** -53 + 2.0 ** -50) * total, (what, c.sumsq, rest)
            assert fences_intact(wbuf, nws) and fences_intact(cbuf, CTL_BYTES), what
    idx = torch.tensor(sorted(set(pos.values())))
    gd[idx.to(DEV)] = float("nan")
    _, ws = fenced(nws)
    _, ctl = new_ctl()
    c = run_stats(gd, gs, 0.0, ws, ctl)
    assert c.nonfinite == len(idx) and c.skip == 1 and (c.applied, c.skipped) == (0, 1)
    gd.fill_(float("inf"))                                                       # every element: the count is n, the sum 0
    c = run_stats(gd, gs, 0.0, ws, ctl)
    assert c.nonfinite == n and c.sumsq == 0.0 and c.norm == 0.0 and (c.applied, c.skipped) == (0, 2)


def test_grad_stats_rejected_calls():
    g = torch.zeros(8, device=DEV)
    wbuf, ws = fenced(ws_bytes(8))
    cbuf, ctl = new_ctl()
    before = cbuf.cpu().clone()
    a = (F(1.0), F(0.0), F(B1), F(B2))
    rejected(lib.rmcl_grad_stats_f32(None, I64(8), *a, P(ws), P(ctl), stream()), "grad_stats")
    rejected(lib.rmcl_grad_stats_f32(P(g), I64(8), *a, None, P(ctl), stream()), "grad_stats")
    rejected(lib.rmcl_grad_stats_f32(P(g), I64(8), *a, P(ws), None, stream()), "grad_stats")
    rejected(lib.rmcl_grad_stats_f32(P(g), I64(6), *a, P(ws), P(ctl), stream()), "grad_stats")
    rejected(lib.rmcl_grad_stats_f32(P(g), I64(0), *a, P(ws), P(ctl), stream()), "grad_stats")
    torch.cuda.synchronize()
    assert torch.equal(cbuf.cpu(), before) and bool((wbuf.cpu() == SENTINEL).all())


# ------------------------------------------------------------------------------------------ 2. guarded AdamW
BIG_4096 = 4096 * 1024 + 1028       # tests/test_step_kernels_gpu.py: beyond one pass of rmcl_adamw_f32's grid (and two of the guarded kernel's)
ADAMW_MULT = [1.0, 10.0, 0.1, 5.0, 0.0]
ADAMW_WD = [0.01, 0.0, 0.1, 0.0, 0.01]
ADAMW_ENDS = [64, 192, 4160, 4096 * 1024 + 192]
ADAMW_EVENTS = [1, 2, "skip", 3, 10000]     # the steps of test_adamw_against_fp64, with one dropped step between steps 2 and 3
LR, EPS, GS = 1e-3, 1e-8, 1.0 / 3.0


def adamw_segments(n, nseg):
    return [n] if nseg == 1 else [min(e, n) for e in ADAMW_ENDS] + [n]


class Fp64AdamW:
    """The float64 formula and its fp32 twin (oracle.rmcl_oracle.adamw_step) on one state."""

    def __init__(self, n, nseg, p0):
        self.ends = adamw_segments(n, nseg)
        self.starts = [0] + self.ends[:-1]
        self.mult32, self.wd32 = [f32(x) for x in ADAMW_MULT[:nseg]], [f32(x) for x in ADAMW_WD[:nseg]]
        seg_of = torch.bucketize(torch.arange(n), torch.tensor(self.ends), right=True)
        assert int(seg_of.max()) < nseg
        self.mult_e, self.wd_e = torch.tensor(self.mult32, dtype=torch.float64)[seg_of], torch.tensor(self.wd32, dtype=torch.float64)[seg_of]
        self.lr, self.b1, self.b2, self.eps = f32(LR), f32(B1), f32(B2), f32(EPS)
        self.p64, self.m64, self.v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        self.p32, self.m32, self.v32 = p0.clone(), torch.zeros(n), torch.zeros(n)

    def step(self, g64, g32, step):
        lr, b1, b2, eps = self.lr, self.b1, self.b2, self.eps
        self.m64 = b1 * self.m64 + (1 - b1) * g64
        self.v64 = b2 * self.v64 + (1 - b2) * g64 * g64
        self.p64 = self.p64 - (lr * self.mult_e) * (1 - b2 ** step) ** 0.5 / (1 - b1 ** step) * self.m64 / (self.v64.sqrt() + eps)
        self.p64 = torch.where(self.wd_e > 0, self.p64 - (lr * self.mult_e) * self.wd_e * self.p64, self.p64)
        for s, e, mu, w in zip(self.starts, self.ends, self.mult32, self.wd32):
            O.adamw_step(self.p32[s:e], g32[s:e], self.m32[s:e], self.v32[s:e], step, lr * mu, w, b1, b2, eps)

    def check(self, p, m, v, what):
        for name, got, ref, twin in (("p", p, self.p64, self.p32), ("m", m, self.m64, self.m32), ("v", v, self.v64, self.v32)):
            got = got.double().cpu()
            assert torch.isfinite(got).all()
            e32 = float((twin.double() - ref).abs().max())
            allowed = ADAMW_FACTOR * max(e32, 2.0 ** -23 * float(ref.abs().max()))
            err = float((got - ref).abs().max())
            PARITY[f"{what}/{name}"] = {"e32": e32, "kernel_dev": err, "allowed": allowed, "ratio": err / allowed}
            assert err <= allowed, (what, name, PARITY[f"{what}/{name}"])


class DeviceAdamW:
    def __init__(self, n, nseg, p0):
        ends = adamw_segments(n, nseg)
        self.n, self.nseg = n, nseg
        self.seg_end = torch.tensor(ends, dtype=torch.int64, device=DEV)
        self.mult = torch.tensor([f32(x) for x in ADAMW_MULT[:nseg]], device=DEV)
        self.wd = torch.tensor([f32(x) for x in ADAMW_WD[:nseg]], device=DEV)
        self.p, self.m, self.v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)

    def plain(self, gd, step, lp):
        check(lib.rmcl_adamw_f32(P(self.p), P(gd), P(self.m), P(self.v), P(self.shadow if lp else None), P(self.seg_end), P(self.mult), P(self.wd),
                                 self.nseg, F(LR), F(B1), F(B2), F(EPS), step, F(GS), I64(self.n), stream()), "adamw")

    def guarded(self, gd, ctl, lp):
        return lib.rmcl_adamw_guarded_f32(P(self.p), P(gd), P(self.m), P(self.v), P(self.shadow if lp else None), P(self.seg_end), P(self.mult),
                                          P(self.wd), self.nseg, F(LR), F(B1), F(B2), F(EPS), F(GS), P(ctl), I64(self.n), stream())

    def state(self):
        return [t.clone() for t in (self.p, self.m, self.v, self.shadow)]


@pytest.mark.parametrize("nseg", [1, 5])
@pytest.mark.parametrize("n", [64, 4160, BIG_4096])
def test_guarded_adamw_against_fp64_and_the_plain_kernel(n, nseg):
    """(a) and (b).  Steps 1, 2, a DROPPED step, 3, then 10000 (ctl.applied set to 9999) on one state, with and without the bf16 shadow."""
    gs = f32(GS)
    p0, g = cpu_randn(n, seed=n % 977 + 1), cpu_randn(n, seed=n % 977 + 2)
    g64, g32 = g.double() * gs, g * torch.tensor(gs)
    ref = Fp64AdamW(n, nseg, p0)
    plain = DeviceAdamW(n, nseg, p0)
    dev = {lp: DeviceAdamW(n, nseg, p0) for lp in (True, False)}
    gd = g.to(DEV)
    bad = gd.clone()
    bad[n // 2] = float("inf")
    ctls = {lp: new_ctl() for lp in (True, False)}                              # (whole buffer, decision block) per optimizer state
    _, ws = fenced(ws_bytes(n))
    for ev in ADAMW_EVENTS:
        if ev == "skip":
            for lp in (True, False):
                ctl = ctls[lp][1]
                before, c0 = dev[lp].state(), L.StepCtl.from_tensor(ctl)
                c = run_stats(bad, gs, 0.0, ws, ctl)
                assert c.skip == 1 and c.nonfinite == 1
                assert (c.applied, c.skipped, c.bc1, c.bc2s) == (c0.applied, c0.skipped + 1, c0.bc1, c0.bc2s) and c0.applied == 2
                check(dev[lp].guarded(bad, ctl, lp), "adamw_guarded")
                for a, b in zip(dev[lp].state(), before):
                    assert same_bits(a, b)                                        # not one byte of p, m, v or the shadow moved
            continue
        step = ev
        ref.step(g64, g32, step)
        plain.plain(gd, step, lp=True)
        for lp in (True, False):
            ctl = ctls[lp][1]
            if step == 10000:
                ctl.copy_(L.StepCtl(applied=9999, skipped=1).to_tensor(DEV))
            c = run_stats(gd, gs, 0.0, ws, ctl)
            # the clean step after the dropped one is step applied + 1 = 3 of the formula, although it is the fourth attempt
            assert (c.skip, c.applied, c.clip_coef, c.skipped) == (0, step, 1.0, 0 if step < 3 else 1)
            assert (c.bc1, c.bc2s) == bias_corrections(step)
            check(dev[lp].guarded(gd, ctl, lp), "adamw_guarded")
        for a, b in zip(dev[True].state()[:3], dev[False].state()[:3]):
            assert torch.equal(a, b), step                                       # p, m, v do not depend on the shadow
        d = dev[True]
        assert same_bits(d.shadow, d.p.to(torch.bfloat16)), step                 # the shadow is bf16 of the kernel's own p
        assert same_bits(d.m, plain.m) and same_bits(d.v, plain.v), step          # (a): m and v are rmcl_adamw_f32's, bit for bit
        p_equal = same_bits(d.p, plain.p)
        what = f"guarded/{n}/{nseg}/step{step}"
        ref.check(d.p, d.m, d.v, what)
        PARITY[what + "/p"]["bit_equal_to_rmcl_adamw_f32"] = p_equal
        print(what, "p bit-equal to rmcl_adamw_f32:", p_equal, {k: round(PARITY[f"{what}/{k}"]["ratio"], 4) for k in "pmv"})
        if not p_equal:                                                          # keep the plain kernel on the guarded state for the next step's m, v
            plain.p.copy_(d.p)
    assert all(fences_intact(buf, CTL_BYTES) for buf, _ in ctls.values())
    if nseg == 5:                                                               # lr_mult = 0: the last segment's weights never move
        s = adamw_segments(n, nseg)[-2]
        assert torch.equal(dev[True].p[s:].cpu(), p0[s:])


@pytest.mark.parametrize("n", [4160, BIG_4096])
def test_guarded_adamw_clipping(n):
    """(c).  max_norm = norm / 2: float64 AdamW on g * grad_scale * coef (coef as the statistics pass wrote it; its own accuracy is
    test_grad_stats_against_fp64's), two steps.  max_norm = 2 norm + 2e-6: coef is exactly 1 and the bits are the unclipped step's."""
    nseg, gs = 5, f32(GS)
    p0, g = cpu_randn(n, seed=n % 977 + 1), cpu_randn(n, seed=n % 977 + 2)
    gd = g.to(DEV)
    norm = gs * float(g.double().norm())
    _, ws = fenced(ws_bytes(n))
    runs = {}
    for name, max_norm in (("off", 0.0), ("half", 0.5 * norm), ("twice", 2.0 * norm + 2e-6)):
        d = DeviceAdamW(n, nseg, p0)
        ref = Fp64AdamW(n, nseg, p0)
        _, ctl = new_ctl()
        for step in (1, 2):
            c = run_stats(gd, gs, max_norm, ws, ctl)
            assert c.skip == 0 and c.applied == step
            assert (c.clip_coef == 1.0) == (name != "half"), (name, c.clip_coef)
            check(d.guarded(gd, ctl, True), "adamw_guarded")
            if name == "half":
                assert abs(c.clip_coef - 0.5) < 1e-5
                coef = float(c.clip_coef)
                ref.step(g.double() * gs * coef, g * torch.tensor(gs) * torch.tensor(coef), step)
                ref.check(d.p, d.m, d.v, f"clip/{n}/step{step}")
                assert same_bits(d.shadow, d.p.to(torch.bfloat16))
        runs[name] = d.state()
    for a, b in zip(runs["twice"], runs["off"]):
        assert same_bits(a, b)
    assert not torch.equal(runs["half"][1], runs["off"][1])                      # (the clipped run did differ: m scales with coef)


def test_guarded_adamw_rejected_calls():
    """(d)."""
    d = DeviceAdamW(64, 1, torch.ones(64))
    g = torch.ones(64, device=DEV)
    _, ctl = new_ctl(applied=1, bc1=0.1, bc2s=0.1, clip_coef=1.0)
    rejected(d.guarded(g, None, True), "adamw_guarded")
    d.n = 62
    rejected(d.guarded(g, ctl, True), "adamw_guarded")
    d.n, d.nseg = 64, 0
    rejected(d.guarded(g, ctl, True), "adamw_guarded")
    d.nseg = 1
    rejected(lib.rmcl_adamw_guarded_f32(None, P(g), P(d.m), P(d.v), None, P(d.seg_end), P(d.mult), P(d.wd), 1, F(LR), F(B1), F(B2), F(EPS), F(GS),
                                        P(ctl), I64(64), stream()), "adamw_guarded")
    torch.cuda.synchronize()
    assert bool((d.p == 1).all()) and bool((d.m == 0).all()) and bool((d.shadow == 0).all())
