"""-m gpu: rmcl_optim_step_f32 (Adam and SGD over the flat arenas, csrc/optim.hip) through the C ABI against float64 on the host.

The sizes, segment tables, steps and tolerance rule are those of tests/test_step_kernels_gpu.py test_adamw_against_fp64: per buffer
(p, m, and v for Adam) |kernel - fp64| <= 4 * max(e32, 2^-23 * max|ref|), e32 = the deviation from float64 of an fp32 CPU twin written
in the kernel's stated order (tests/optim_rules_ref.py, from the comment in include/rmcl.h), on the whole buffer and on the 64 elements
either side of every segment end.  BIG_4096 lies just beyond one pass of the kernel's 4096-block grid, with a segment end inside the
second pass.
  plain     steps 1, 2, 3 on one state, then step 10000, grad_scale = 1/3; with and without the bf16 shadow (p, m, v identical, the
            shadow bit-equal to bf16(p)); the lr_mult = 0 segment keeps p0's bits
  guarded   the events [1, 2, "skip", 3, 10000] of tests/test_guarded_step_kernels_gpu.py: a NaN in the gradient, the decision taken
            by rmcl_grad_stats_f32; a skipped call changes no byte; unclipped, p, m and v are the plain form's bits
  clipping  max_norm = norm / 2 against float64 on g * grad_scale * coef (coef as written in ctl); max_norm = 2 norm + 2e-6 gives the
            unclipped bits; a second run of the same calls gives the same bytes
  eps       Adam with |g| ~ 1e-9: eps dominates the denominator, and the update with eps in HF AdamW's place is off by more than the bound
  rejected  n % 4 != 0, nseg = 0, an unknown rule, SGD with a v pointer, Adam without one: -1 and untouched buffers
Measured ratios go to the file named by RMCL_OPTIM_RULES_PARITY_OUT when set (profiles/optim_rules_parity.json is such a dump)."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream  # noqa: E402
from tests import optim_rules_ref as R  # noqa: E402
from tests.optim_rules_ref import f32  # noqa: E402

PARITY = {}
ADAMW_FACTOR = 4.0
GUARD = 256
SENTINEL = 0xA5
CTL_BYTES = C.sizeof(L.StepCtl)
BIG_4096 = 4096 * 1024 + 1028       # one pass of the 4096-block grid covers 4096 * 1024 elements: the grid-stride loop iterates
ADAMW_MULT = [1.0, 10.0, 0.1, 5.0, 0.0]
ADAMW_WD = [0.01, 0.0, 0.1, 0.0, 0.01]
ADAMW_ENDS = [64, 192, 4160, 4096 * 1024 + 192]
STEPS = [1, 2, 3, 10000]
EVENTS = [1, 2, "skip", 3, 10000]
LR, GS = 1e-3, 1.0 / 3.0
RULES = {"adam": (R.ADAM, R.ADAM_BETAS[0], R.ADAM_BETAS[1], R.ADAM_EPS), "sgd": (R.SGD, R.SGD_MOMENTUM, 0.0, 0.0)}   # code, beta1, beta2, eps
BUFFERS = {"adam": "pmv", "sgd": "pm"}


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_OPTIM_RULES_PARITY_OUT")
    if out and PARITY:
        with open(out, "w") as f:
            json.dump({"adamw_factor": ADAMW_FACTOR, "cases": PARITY}, f, indent=1, sort_keys=True)


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
    buf = torch.full((2 * GUARD + nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def fences_intact(buf, nbytes):
    b = buf.cpu()
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + nbytes:] == SENTINEL).all())


def new_ctl(**fields):
    buf, ctl = fenced(CTL_BYTES)
    ctl.copy_(L.StepCtl(**fields).to_tensor(DEV))
    return buf, ctl


def stats_ws(n):
    return fenced(int(lib.rmcl_grad_stats_ws_bytes(I64(n))))[1]


def run_stats(rule, gd, gs, max_norm, ws, ctl):
    _, b1, b2, _ = RULES[rule]
    check(lib.rmcl_grad_stats_f32(P(gd), I64(gd.numel()), F(gs), F(max_norm), F(b1), F(b2), P(ws), P(ctl), stream()), "grad_stats")
    return L.StepCtl.from_tensor(ctl)


def segments(n, nseg):
    """Exclusive segment ends; nseg = 5 on a short arena leaves EMPTY trailing segments."""
    return [n] if nseg == 1 else [min(e, n) for e in ADAMW_ENDS] + [n]


class Reference:
    """The float64 rule and its fp32 twin (tests/optim_rules_ref.py rule_step) on one state."""

    def __init__(self, rule, n, ends, mult, wd, p0):
        self.rule, self.code = rule, RULES[rule][0]
        self.ends = ends
        self.mult32, self.wd32 = [f32(x) for x in mult], [f32(x) for x in wd]
        seg_of = torch.bucketize(torch.arange(n), torch.tensor(ends), right=True)      # first segment with end > e
        assert int(seg_of.max()) < len(mult)
        self.lr, self.b1, self.b2, self.eps = f32(LR), f32(RULES[rule][1]), f32(RULES[rule][2]), f32(RULES[rule][3])
        self.slr64, self.wd64 = self.lr * torch.tensor(self.mult32, dtype=torch.float64)[seg_of], torch.tensor(self.wd32, dtype=torch.float64)[seg_of]
        self.slr32, self.wd32e = torch.tensor(self.lr) * torch.tensor(self.mult32)[seg_of], torch.tensor(self.wd32)[seg_of]
        self.s64 = {"p": p0.double(), "m": torch.zeros(n, dtype=torch.float64), "v": torch.zeros(n, dtype=torch.float64)}
        self.s32 = {"p": p0.clone(), "m": torch.zeros(n), "v": torch.zeros(n)}
        self.edges = sorted({e for e in ends if e < n})

    def step(self, g64, g32, t):
        bc1, bc2s = R.bias_corrections(RULES[self.rule][1], RULES[self.rule][2], t)
        for s, g, slr, wd in ((self.s64, g64, self.slr64, self.wd64), (self.s32, g32, self.slr32, self.wd32e)):
            R.rule_step(self.code, s["p"], g, s["m"], s["v"], slr, wd, self.b1, self.b2, self.eps, bc1, bc2s)

    def allowed(self, name):
        e32 = float((self.s32[name].double() - self.s64[name]).abs().max())
        return e32, ADAMW_FACTOR * max(e32, 2.0 ** -23 * float(self.s64[name].abs().max()))

    def check(self, dev, what):
        for name in BUFFERS[self.rule]:
            got, ref = getattr(dev, name).double().cpu(), self.s64[name]
            assert torch.isfinite(got).all()
            e32, allowed = self.allowed(name)
            err = (got - ref).abs()
            fig = {"e32": e32, "kernel_dev": float(err.max()), "allowed": allowed, "ratio": float(err.max()) / allowed}
            PARITY[f"{what}/{name}"] = fig
            print(what, name, fig)
            for edge in self.edges:                                              # an off-by-one segment changes these by a factor
                lo, hi = float(err[edge - 64:edge].max()), float(err[edge:edge + 64].max())
                assert lo <= allowed, f"{what} {name}: the 64 elements BELOW the segment end {edge}: {lo} > {allowed}"
                assert hi <= allowed, f"{what} {name}: the 64 elements FROM the segment end {edge} on: {hi} > {allowed}"
            assert float(err.max()) <= allowed, (what, name, fig)


class Device:
    def __init__(self, rule, n, ends, mult, wd, p0):
        self.rule, self.n, self.nseg = rule, n, len(ends)
        self.seg_end = torch.tensor(ends, dtype=torch.int64, device=DEV)
        self.mult = torch.tensor([f32(x) for x in mult], device=DEV)
        self.wd = torch.tensor([f32(x) for x in wd], device=DEV)
        self.p, self.m = p0.to(DEV), torch.zeros(n, device=DEV)
        self.v = torch.zeros(n, device=DEV) if rule == "adam" else None
        self.shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)

    def call(self, gd, step, lp, ctl=None, code=None, v="own"):
        """ctl None: the plain form at `step`; ctl given: the guarded form (step is ignored: -7 is handed over)."""
        rc, b1, b2, eps = RULES[self.rule]
        return lib.rmcl_optim_step_f32(rc if code is None else code, P(self.p), P(gd), P(self.m), P(self.v if v == "own" else v),
                                       P(self.shadow if lp else None), P(self.seg_end), P(self.mult), P(self.wd), self.nseg, F(LR), F(b1), F(b2),
                                       F(eps), step if ctl is None else -7, F(GS), P(ctl), I64(self.n), stream())

    def state(self):
        return [t.clone() for t in (self.p, self.m, self.v, self.shadow) if t is not None]

    def moments(self):
        return [t for t in (self.p, self.m, self.v) if t is not None]


def tables(nseg):
    return ADAMW_MULT[:nseg], ADAMW_WD[:nseg]


def inputs(n):
    return cpu_randn(n, seed=n % 977 + 1), cpu_randn(n, seed=n % 977 + 2)


# ------------------------------------------------------------------------------------------ 1. the plain form
@pytest.mark.parametrize("nseg", [1, 5])
@pytest.mark.parametrize("n", [64, 4160, BIG_4096])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_rule_against_fp64(rule, n, nseg):
    gs = f32(GS)
    ends, (mult, wd) = segments(n, nseg), tables(nseg)
    p0, g = inputs(n)
    g64, g32 = g.double() * gs, g * torch.tensor(gs)
    ref = Reference(rule, n, ends, mult, wd, p0)
    dev = {lp: Device(rule, n, ends, mult, wd, p0) for lp in (True, False)}
    gd = g.to(DEV)
    for step in STEPS:
        ref.step(g64, g32, step)
        for lp in (True, False):
            check(dev[lp].call(gd, step, lp), "optim_step")
        for a, b in zip(dev[True].moments(), dev[False].moments()):
            assert torch.equal(a, b), step                                       # p, m, v do not depend on the shadow
        d = dev[True]
        assert same_bits(d.shadow, d.p.to(torch.bfloat16)), step                 # the shadow is bf16 of the kernel's own p
        assert not bool(dev[False].shadow.any())                                 # (and is not written when not asked for)
        ref.check(d, f"{rule}/{n}/{nseg}/step{step}")
    assert torch.equal(gd.cpu(), g)
    if nseg == 5:                                                                # lr_mult = 0: the last segment's weights never move
        s = ends[-2]
        assert torch.equal(dev[True].p[s:].cpu(), p0[s:])
        if s < n:
            assert float(dev[True].m[s:].abs().max()) > 0                        # (its moments do: the gradient is not zero there)


# ------------------------------------------------------------------------------------------ 2. the guarded form
@pytest.mark.parametrize("nseg", [1, 5])
@pytest.mark.parametrize("n", [64, 4160, BIG_4096])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_guarded_rule_against_fp64_and_the_plain_form(rule, n, nseg):
    """Steps 1, 2, a DROPPED step, 3, then 10000 (ctl.applied set to 9999) on one state, with and without the bf16 shadow."""
    gs = f32(GS)
    ends, (mult, wd) = segments(n, nseg), tables(nseg)
    p0, g = inputs(n)
    g64, g32 = g.double() * gs, g * torch.tensor(gs)
    ref = Reference(rule, n, ends, mult, wd, p0)
    plain = Device(rule, n, ends, mult, wd, p0)
    dev = {lp: Device(rule, n, ends, mult, wd, p0) for lp in (True, False)}
    gd = g.to(DEV)
    bad = gd.clone()
    bad[n // 2] = float("nan")
    ctls = {lp: new_ctl() for lp in (True, False)}
    ws = stats_ws(n)
    for ev in EVENTS:
        if ev == "skip":
            for lp in (True, False):
                ctl = ctls[lp][1]
                before, c0 = dev[lp].state(), L.StepCtl.from_tensor(ctl)
                c = run_stats(rule, bad, gs, 0.0, ws, ctl)
                assert c.skip == 1 and c.nonfinite == 1
                assert (c.applied, c.skipped, c.bc1, c.bc2s) == (c0.applied, c0.skipped + 1, c0.bc1, c0.bc2s) and c0.applied == 2
                check(dev[lp].call(bad, 0, lp, ctl=ctl), "optim_step")
                for a, b in zip(dev[lp].state(), before):
                    assert same_bits(a, b)                                        # not one byte of p, m, v or the shadow moved
            continue
        step = ev
        ref.step(g64, g32, step)
        check(plain.call(gd, step, True), "optim_step")
        for lp in (True, False):
            ctl = ctls[lp][1]
            if step == 10000:
                ctl.copy_(L.StepCtl(applied=9999, skipped=1).to_tensor(DEV))
            c = run_stats(rule, gd, gs, 0.0, ws, ctl)
            # the clean step after the dropped one is step applied + 1 = 3 of the formula, although it is the fourth attempt
            assert (c.skip, c.applied, c.clip_coef, c.skipped) == (0, step, 1.0, 0 if step < 3 else 1)
            assert (c.bc1, c.bc2s) == R.bias_corrections(RULES[rule][1], RULES[rule][2], step)
            check(dev[lp].call(gd, step, lp, ctl=ctl), "optim_step")
        for a, b in zip(dev[True].moments(), dev[False].moments()):
            assert torch.equal(a, b), step
        d = dev[True]
        assert same_bits(d.shadow, d.p.to(torch.bfloat16)), step
        for name, a, b in zip("pmv", d.moments(), plain.moments()):
            assert same_bits(a, b), (step, name)                                 # unclipped: the plain form's bits
        assert same_bits(d.shadow, plain.shadow), step
        ref.check(d, f"guarded/{rule}/{n}/{nseg}/step{step}")
    assert all(fences_intact(buf, CTL_BYTES) for buf, _ in ctls.values())
    if nseg == 5:
        s = ends[-2]
        assert torch.equal(dev[True].p[s:].cpu(), p0[s:])


@pytest.mark.parametrize("n", [4160, BIG_4096])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_guarded_rule_clipping(rule, n):
    """max_norm = norm / 2: the float64 rule on g * grad_scale * coef (coef as the statistics pass wrote it; its own accuracy is
    tests/test_guarded_step_kernels_gpu.py test_grad_stats_against_fp64's), two steps.  max_norm = 2 norm + 2e-6: coef is exactly 1 and
    the bits are the unclipped step's.  The clipped run a second time: the same bytes."""
    nseg, gs = 5, f32(GS)
    ends, (mult, wd) = segments(n, nseg), tables(nseg)
    p0, g = inputs(n)
    gd = g.to(DEV)
    norm = gs * float(g.double().norm())
    ws = stats_ws(n)
    runs = {}
    for name, max_norm in (("off", 0.0), ("half", 0.5 * norm), ("half_again", 0.5 * norm), ("twice", 2.0 * norm + 2e-6)):
        d = Device(rule, n, ends, mult, wd, p0)
        ref = Reference(rule, n, ends, mult, wd, p0)
        _, ctl = new_ctl()
        for step in (1, 2):
            c = run_stats(rule, gd, gs, max_norm, ws, ctl)
            assert c.skip == 0 and c.applied == step
            assert (c.clip_coef == 1.0) == (not name.startswith("half")), (name, c.clip_coef)
            check(d.call(gd, step, True, ctl=ctl), "optim_step")
            if name == "half":
                assert abs(c.clip_coef - 0.5) < 1e-5
                coef = float(c.clip_coef)
                ref.step(g.double() * gs * coef, g * torch.tensor(gs) * torch.tensor(coef), step)
                ref.check(d, f"clip/{rule}/{n}/step{step}")
                assert same_bits(d.shadow, d.p.to(torch.bfloat16))
        runs[name] = d.state()
    for a, b in zip(runs["twice"], runs["off"]):
        assert same_bits(a, b)
    for a, b in zip(runs["half_again"], runs["half"]):
        assert same_bits(a, b)
    assert not torch.equal(runs["half"][1], runs["off"][1])                      # (the clipped run did differ: m scales with coef)


# ------------------------------------------------------------------------------------------ 3. where Adam's eps goes
def test_adam_adds_eps_after_the_bias_correction():
    """|g| * grad_scale in [0.5e-9, 1.5e-9] against eps = 1e-8, one segment, no weight decay (the coupled decay would put 0.01 p into the
    gradient), step 1 and step 2.  The kernel meets the bound against torch's placement, and p computed with eps in HF AdamW's place
    (from the same moments) lies farther than the bound from the kernel's p at EVERY element (tests/test_optim_rules_cpu.py
    test_the_eps_placements_differ_where_eps_dominates is the float64 statement of that gap)."""
    n, gs = 4160, f32(GS)
    gen = torch.Generator(device="cpu").manual_seed(5)
    p0 = cpu_randn(n, seed=6)
    mag = (0.5 + torch.rand(n, generator=gen)) * 1e-9 / gs
    g = torch.where(torch.rand(n, generator=gen) < 0.5, -mag, mag)
    g64, g32 = g.double() * gs, g * torch.tensor(gs)
    ref = Reference("adam", n, [n], [1.0], [0.0], p0)
    d = Device("adam", n, [n], [1.0], [0.0], p0)
    gd = g.to(DEV)
    for step in (1, 2):
        bc1, bc2s = R.bias_corrections(*R.ADAM_BETAS, step)
        hf = R.hf_adamw_p64(ref.s64["p"], g64, ref.s64["m"], ref.s64["v"], ref.slr64, ref.b1, ref.b2, ref.eps, bc1, bc2s)
        ref.step(g64, g32, step)
        check(d.call(gd, step, True), "optim_step")
        ref.check(d, f"eps/adam/{n}/step{step}")
        _, allowed = ref.allowed("p")
        gap = float((ref.s64["p"] - hf).abs().min())
        assert gap > 10 * allowed, (gap, allowed)                                # the two placements are told apart on this input
        off = float((d.p.double().cpu() - hf).abs().min())
        PARITY[f"eps/adam/{n}/step{step}/p"]["distance_from_hf_placement"] = off
        assert off > allowed, (step, off, allowed)


# ------------------------------------------------------------------------------------------ 4. rejected calls
def test_rejected_calls_leave_the_buffers_alone():
    g = torch.ones(64, device=DEV)
    _, ctl = new_ctl(applied=1, bc1=0.1, bc2s=0.1, clip_coef=1.0)
    adam, sgd = Device("adam", 64, [64], [1.0], [0.0], torch.ones(64)), Device("sgd", 64, [64], [1.0], [0.0], torch.ones(64))
    spare = torch.zeros(64, device=DEV)
    for d in (adam, sgd):
        for c in (None, ctl):
            d.n = 62
            rejected(d.call(g, 1, True, ctl=c), "optim_step")                    # n % 4 != 0
            d.n = 0
            rejected(d.call(g, 1, True, ctl=c), "optim_step")
            d.n, d.nseg = 64, 0
            rejected(d.call(g, 1, True, ctl=c), "optim_step")                    # nseg = 0
            d.nseg = 1
            for code in (0, 3, -1):
                rejected(d.call(g, 1, True, ctl=c, code=code), "unknown rule")
        rejected(d.call(g, 0, True), "step >= 1")                                # the plain form counts steps from 1
        rejected(d.call(None, 1, True), "NULL")
    rejected(sgd.call(g, 1, True, v=spare), "v must be NULL")                    # SGD keeps no second moment
    rejected(sgd.call(g, 1, True, ctl=ctl, v=spare), "v must be NULL")
    rejected(adam.call(g, 1, True, v=None), "Adam needs v")
    torch.cuda.synchronize()
    for d in (adam, sgd):
        assert bool((d.p == 1).all()) and bool((d.m == 0).all()) and bool((d.shadow == 0).all())
    assert bool((adam.v == 0).all()) and bool((spare == 0).all())
