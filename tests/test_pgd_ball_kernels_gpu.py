"""-m gpu: rmcl_pgd_step_ball, rmcl_pgd_random_start and rmcl_pgd_keep_worst (csrc/pgd_ball.hip) through the C ABI against the float64 /
integer model of tests/pgd_ball_ref.py, at the grid arms of the existing PGD kernels (fewer blocks than partial slots, one element
group on either side of the 64-block cap, the training step's 144 x 3072), for both gradient and both operand types.

Every element must lie within the allowance the model derives (see its docstring); the facts that hold exactly are asserted exactly:
pad slots, the L-inf clamp values, the box on the operand, untouched guard words around every buffer, scratch slots beyond the launch's
block count, byte-identical repeats, and the default arm's equality with rmcl_pgd_step_fused.

Two bounds are this file's own.  L-inf ball WITH a box: delta_new = fl(x - base) with x = fl(base + t'), so |delta_new| can pass eps by the
rounding of the pixel x, at most 2^-24 |x| (x - base itself is then exact or rounds by less): asserted as eps + 2^-23 max(|x|, |base|).
Sample 2 (all-zero gradient) keeps its delta bit for bit only without a box, for the same reason.
Measured deviation / allowance ratios are collected in PARITY, reduced per arm (the largest over the sizes and the gradient / operand
types: `per_arm`) and written to the file named by RMCL_PGD_BALL_PARITY_OUT when set (profiles/pgd_ball_parity.json is such a dump)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream, tdt  # noqa: E402
from tests import pgd_ball_ref as R  # noqa: E402

PARITY = {}
B = 3
PER = [4, 1028, 3072, 3 * 3072, 64 * 1024 - 4, 64 * 1024 + 4, 144 * 3072]
GUARD = 64                                       # guard elements on each side of every buffer
EPS_LINF, LR_NORMALISED, LR_SIGN = 0.005, 0.01, 0.002
EPS_L2 = 1.0                                     # an L2 radius of pixel scale: 1.0 on [-1, 1] images is 0.5 on [0, 1] ones
LR_L2 = 0.6 * EPS_L2
BOX = (-1.0, 1.0)
THREATS = {"normalised_linf": (L.PGD_DIR_NORMALISED, L.PGD_BALL_LINF, LR_NORMALISED, EPS_LINF),
           "sign_linf": (L.PGD_DIR_SIGN, L.PGD_BALL_LINF, LR_SIGN, EPS_LINF),
           "l2_l2": (L.PGD_DIR_L2, L.PGD_BALL_L2, LR_L2, EPS_L2)}
SCRATCH_FILL = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_PGD_BALL_PARITY_OUT")
    if out and PARITY:
        with open(out, "w") as f:
            json.dump({"allowed": {"*_over_allowed": 1.0, "l2_norm_over_eps_max": 1 + 2.0 ** -22}, "arms": per_arm(PARITY)}, f, indent=1, sort_keys=True)


def per_arm(cases):
    """PARITY reduced to one entry per arm: keys "step/<threat>/<size>/<g type>/<o type>/<box>/<valid>/<eps>/<zero>" and
    "start_l2/<size>/<o type>/<box>/<valid>" lose their size and type fields; every ratio becomes the largest of the arm's cases."""
    arms = {}
    for key, fig in cases.items():
        parts = key.split("/")
        arm = "/".join(parts[:2] + parts[5:]) if parts[0] == "step" else "/".join(parts[:1] + parts[3:])
        a = arms.setdefault(arm, {"cases": 0})
        a["cases"] += 1
        for k, v in fig.items():
            if k.endswith("over_allowed"):
                a[k] = max(a.get(k, 0.0), v)
            elif k == "l2_norm_over_eps":
                a["l2_norm_over_eps_max"] = max(a.get("l2_norm_over_eps_max", 0.0), max(v))
    return arms


def cpu_randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def guarded(t, fill=None):
    """A device copy of the CPU tensor t with GUARD elements of a known pattern before and behind it: (view, whole buffer, pattern)."""
    n = t.numel()
    pat = {torch.float32: 1.0e30, torch.bfloat16: 1.0e30, torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}[t.dtype] if fill is None else fill
    buf = torch.full((n + 2 * GUARD,), pat, dtype=t.dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    return view, buf, pat


def guards_intact(buf, pat):
    want = torch.full((GUARD,), pat, dtype=buf.dtype, device=buf.device)
    return torch.equal(buf[:GUARD], want) and torch.equal(buf[-GUARD:], want)


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def blocks(per):
    return min((per + 1023) // 1024, 64)


def scratch_bytes(b=B):
    n = int(lib.rmcl_pgd_ball_scratch_bytes(b))
    assert n == b * (2 * 64 * 8 + 64 * 4)
    return n


def scratch_untouched_beyond(scr, per, b=B):
    """slots at or beyond the launch's block count, in all three partial arrays, still hold the fill pattern"""
    raw = scr.cpu().numpy()
    sq = raw[: b * 2 * 64 * 8].reshape(b, 2, 64, 8)
    am = raw[b * 2 * 64 * 8:].reshape(b, 64, 4)
    nb = blocks(per)
    return bool((sq[:, :, nb:] == SCRATCH_FILL).all()) and bool((am[:, nb:] == SCRATCH_FILL).all())


def ragged_valid(per):
    """full, a middle count (a multiple of 3072 where the size allows, else of 4), 0 = an all-pad sample"""
    mid = (per // 2 // 3072) * 3072 if per >= 2 * 3072 else (per // 8) * 4
    return [per, mid, 0]


@functools.lru_cache(maxsize=None)
def inputs(per, dt, ball):
    """g [3, per] in the gradient type, delta0 and base [3, per] f32, all on the CPU.  g as in tests/test_step_kernels_gpu.py: sample 0's
    largest |g| in its last four elements, sample 1's in its first four, sample 2 all zero.  base: uniform in (-0.9, 0.9) with 6 % of
    the elements on each edge of the box (saturated pixels), so that a step pointing outward is clamped.  L2: ||delta0|| = 0.9 / 0.3 /
    0.5 eps, so that with lr = 0.6 eps sample 0 leaves the ball and samples 1 and 2 stay inside."""
    g = cpu_randn(B, per, seed=per % 9973 + 11)
    signs = torch.tensor([1.0, -1.0, -1.0, 1.0])
    g[0, -4:] = (g[0].abs().max() + 0.5) * signs
    g[1, :4] = -(g[1].abs().max() + 0.5) * signs
    g[2] = 0
    g = g.to(tdt(dt))
    d = cpu_randn(B, per, seed=per % 9973 + 12)
    if ball == L.PGD_BALL_LINF:
        delta0 = (d * 0.002).clamp(-EPS_LINF, EPS_LINF)
    else:
        gf = g[0].float()
        if float(d[0] @ gf) < 0:                                                    # sample 0 does not step back towards the centre
            d[0] -= 2 * (d[0] @ gf) / (gf @ gf) * gf
        delta0 = d / d.norm(dim=1, keepdim=True) * torch.tensor([[0.9], [0.3], [0.5]]) * EPS_L2
    u = torch.rand(B, per, generator=torch.Generator(device="cpu").manual_seed(per % 9973 + 13))
    base = (cpu_randn(B, per, seed=per % 9973 + 14).mul(0.4)).clamp(-0.9, 0.9)
    base[u < 0.06] = -1.0
    base[u > 0.94] = 1.0
    return g, delta0.float().contiguous(), base.float().contiguous()


def np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def run_step(g, delta0, base, dt, odt, per, direction, ball, lr, eps, box, valid, zero, want_scratch=False):
    gd, gbuf, gpat = guarded(g)
    d0 = torch.full_like(delta0, float("nan")) if zero else delta0           # (DELTA_ZERO must not read the buffer)
    dd, dbuf, dpat = guarded(d0)
    bd, bbuf, bpat = guarded(base)
    od, obuf, opat = guarded(torch.zeros(B, per, dtype=tdt(odt)))
    sc, sbuf, spat = guarded(torch.full((scratch_bytes(),), SCRATCH_FILL, dtype=torch.uint8))
    vd = vbuf = vpat = None
    if valid is not None:
        vd, vbuf, vpat = guarded(torch.tensor(valid, dtype=torch.int32))
    lo, hi = box if box is not None else (0.0, 0.0)
    check(lib.rmcl_pgd_step_ball(P(gd), dt, P(dd), P(sc), P(vd), B, I64(per), F(lr), F(eps), direction, ball, F(lo), F(hi), P(bd), P(od), odt,
                                 L.PGD_DELTA_ZERO if zero else 0, stream()), "pgd_step_ball")
    torch.cuda.synchronize()
    assert guards_intact(gbuf, gpat) and guards_intact(dbuf, dpat) and guards_intact(bbuf, bpat) and guards_intact(obuf, opat)
    assert guards_intact(sbuf, spat) and (vbuf is None or guards_intact(vbuf, vpat))
    assert torch.equal(bits(gd), bits(g.to(DEV))) and torch.equal(bd, base.to(DEV))              # inputs are read only
    assert scratch_untouched_beyond(sc, per)
    return (dd.clone(), od.clone(), sc.clone()) if want_scratch else (dd.clone(), od.clone())


def check_step(what, got_d, got_o, ref, base, odt, ball, eps, box, zero_grad_row_exact, delta0):
    gd, go = np64(got_d), np64(got_o)
    mask, pads = ref["mask"], ~ref["mask"]
    assert np.isfinite(gd).all() and np.isfinite(go).all(), what
    dev_d, dev_o = np.abs(gd - ref["delta"]), np.abs(go - ref["x"])
    fig = {"delta_max_dev": float(dev_d.max()), "delta_dev_over_allowed": float((dev_d / np.maximum(ref["allowed_delta"], 1e-300))[mask].max(initial=0.0)),
           "operand_max_dev": float(dev_o.max()), "operand_dev_over_allowed": float((dev_o / np.maximum(ref["allowed_x"], 1e-300))[mask].max(initial=0.0))}
    eps32 = ref["eps"]
    if ball == L.PGD_BALL_L2 and eps32 > 0:
        nrm = np.sqrt((gd * gd).sum(axis=1))
        fig["l2_norm_over_eps"] = [float(v) for v in nrm / eps32]
    print(what, fig)
    PARITY[what] = fig
    assert (dev_d <= ref["allowed_delta"]).all(), (what, fig)
    assert (dev_o <= ref["allowed_x"]).all(), (what, fig)
    # pad slots: delta = 0 and operand = cast(base), exactly
    assert (gd[pads] == 0).all(), what
    want_pad = base.to(tdt(odt)).to(DEV)
    pm = torch.from_numpy(pads).to(DEV)
    assert torch.equal(bits(got_o)[pm], bits(want_pad)[pm]), what
    if box is not None:                                                                           # the operand lies in the box, exactly
        assert (go[mask] >= box[0]).all() and (go[mask] <= box[1]).all(), what
    if ball == L.PGD_BALL_LINF and eps32 > 0:
        if box is None:
            hi, lo = ref["delta"] == eps32, ref["delta"] == -eps32
            assert (gd[hi] == eps32).all() and (gd[lo] == -eps32).all() and np.abs(gd).max() <= eps32, what
        else:
            assert (np.abs(gd) <= eps32 + 2.0 ** -23 * np.maximum(np.abs(ref["x"]), np.abs(np64(base)))).all(), what
    if ball == L.PGD_BALL_L2 and eps32 > 0:
        assert (nrm <= eps32 * (1 + 2.0 ** -22)).all(), (what, fig)
    if zero_grad_row_exact:
        assert np.array_equal(gd[2], np64(delta0)[2]), what                                       # all-zero gradient: nothing moves
    return fig


@pytest.mark.parametrize("dt,odt", [(L.F32, L.F32), (L.F32, L.BF16), (L.BF16, L.F32), (L.BF16, L.BF16)])
@pytest.mark.parametrize("per", PER)
def test_step_ball_against_fp64(per, dt, odt):
    tag = f"{per}/g{'bf16' if dt else 'f32'}/o{'bf16' if odt else 'f32'}"
    for name, (direction, ball, lr, eps) in THREATS.items():
        g, delta0, base = inputs(per, dt, ball)
        g64, d64, b64 = np64(g), np64(delta0), np64(base)
        arms = [(box, valid, eps, False) for box in (None, BOX) for valid in (None, ragged_valid(per))]
        arms += [(None, None, 0.0, False), (None, None, eps, True)]                               # eps = 0; DELTA_ZERO
        for box, valid, e, zero in arms:
            ref = R.step_ball(g64, d64, lr, e, direction, ball, base=b64, box=box, valid=valid, delta_zero=zero, bf16_operand=odt == L.BF16)
            m = ref["mask"]
            if ball == L.PGD_BALL_L2 and e > 0 and not zero:                                      # out of the ball / inside / zero gradient
                assert ref["scale"][0] < 1.0 and ref["scale"][1] == 1.0 and ref["scale"][2] == 1.0
            if box is not None and per >= 3072:                                                   # the input exercises both box edges (valid elements)
                raw = ref["raw"]
                assert (raw > box[1])[m].mean() >= 0.02 and (raw < box[0])[m].mean() >= 0.02
                assert ((raw >= box[0]) & (raw <= box[1]))[m].mean() >= 0.5
            what = f"step/{name}/{tag}/box{int(box is not None)}/valid{int(valid is not None)}/eps{int(e > 0)}/zero{int(zero)}"
            got_d, got_o, scr = run_step(g, delta0, base, dt, odt, per, direction, ball, lr, e, box, valid, zero, want_scratch=True)
            exact_row = box is None and valid is None and not zero
            check_step(what, got_d, got_o, ref, base, odt, ball, e, box, exact_row, delta0)
            if e == 0 and ball == L.PGD_BALL_LINF and direction == L.PGD_DIR_NORMALISED:
                assert float(got_d.abs().max()) > EPS_LINF                                        # (it really was not clamped)
            if True:                                                                              # a second call writes identical bytes
                d2, o2, s2 = run_step(g, delta0, base, dt, odt, per, direction, ball, lr, e, box, valid, zero, want_scratch=True)
                assert torch.equal(bits(d2), bits(got_d)) and torch.equal(bits(o2), bits(got_o)) and torch.equal(s2, scr), what


@pytest.mark.parametrize("dt,odt", [(L.F32, L.F32), (L.F32, L.BF16), (L.BF16, L.F32), (L.BF16, L.BF16)])
@pytest.mark.parametrize("per", PER)
def test_default_arm_equals_the_fused_step_bitwise(per, dt, odt):
    """normalised / L-inf / no box / no valid = rmcl_pgd_step_fused without SUM_PREV, delta and operand, with and without DELTA_ZERO."""
    g, delta0, base = inputs(per, dt, L.PGD_BALL_LINF)
    gdev, bdev = g.to(DEV), base.to(DEV)
    for zero in (False, True):
        got_d, got_o = run_step(g, delta0, base, dt, odt, per, L.PGD_DIR_NORMALISED, L.PGD_BALL_LINF, LR_NORMALISED, EPS_LINF, None, None, zero)
        delta = torch.full((B, per), float("nan"), device=DEV) if zero else delta0.to(DEV)
        out = torch.empty(B, per, dtype=tdt(odt), device=DEV)
        amax = torch.empty(64 * B, dtype=torch.int32, device=DEV)
        check(lib.rmcl_pgd_step_fused(P(gdev), dt, P(delta), P(amax), B, I64(per), F(LR_NORMALISED), F(EPS_LINF), P(bdev), P(out), odt,
                                      L.PGD_DELTA_ZERO if zero else 0, stream()), "pgd_step_fused")
        assert torch.equal(bits(got_d), bits(delta)) and torch.equal(bits(got_o), bits(out)), (per, zero)


# ------------------------------------------------------------------------------------------ random start
def run_start(per, b, sample0, seed, eps, ball, base, box, valid, odt):
    dd, dbuf, dpat = guarded(torch.full((b, per), float("nan")))
    od, obuf, opat = guarded(torch.zeros(b, per, dtype=tdt(odt)))
    sc, sbuf, spat = guarded(torch.full((scratch_bytes(b),), SCRATCH_FILL, dtype=torch.uint8))
    bd, bbuf, bpat = guarded(base)
    vd = None
    if valid is not None:
        vd, vbuf, vpat = guarded(torch.tensor(valid, dtype=torch.int32))
    lo, hi = box if box is not None else (0.0, 0.0)
    check(lib.rmcl_pgd_random_start(P(dd), P(sc), P(vd), b, I64(per), sample0, seed, F(eps), ball, F(lo), F(hi), P(bd), P(od), odt, stream()),
          "pgd_random_start")
    torch.cuda.synchronize()
    assert guards_intact(dbuf, dpat) and guards_intact(obuf, opat) and guards_intact(sbuf, spat) and guards_intact(bbuf, bpat)
    assert valid is None or guards_intact(vbuf, vpat)
    assert scratch_untouched_beyond(sc, per, b) and torch.equal(bd, base.to(DEV))
    return dd.clone(), od.clone()


@pytest.mark.parametrize("odt", [L.F32, L.BF16])
@pytest.mark.parametrize("per", PER)
def test_random_start_linf_is_the_numpy_restatement_bit_for_bit(per, odt):
    base = inputs(per, L.F32, L.PGD_BALL_LINF)[2]
    for box in (None, BOX):
        for valid in (None, ragged_valid(per)):
            got_d, got_o = run_start(per, B, 5, 1234, EPS_LINF, L.PGD_BALL_LINF, base, box, valid, odt)
            want_d, want_x = R.random_start_linf_f32(B, per, 5, 1234, EPS_LINF, base=base.numpy(), box=box, valid=valid)
            assert np.array_equal(got_d.cpu().numpy().view(np.uint32), want_d.view(np.uint32)), (per, box, valid)
            assert torch.equal(bits(got_o), bits(torch.from_numpy(want_x).to(tdt(odt)).to(DEV))), (per, box, valid)
            if box is None and valid is None and per >= 3072:
                d = got_d.double()
                assert float(d.abs().max()) <= R.f32(EPS_LINF) and abs(float(d.mean())) < 0.05 * EPS_LINF      # fills the cube
                assert abs(float((d * d).mean()) - R.f32(EPS_LINF) ** 2 / 3) < 0.05 * EPS_LINF ** 2
    other = run_start(per, B, 5, 1235, EPS_LINF, L.PGD_BALL_LINF, base, None, None, odt)[0]
    same = run_start(per, B, 5, 1234, EPS_LINF, L.PGD_BALL_LINF, base, None, None, odt)[0]
    assert not torch.equal(other, same)                                                                        # another seed, another start


@pytest.mark.parametrize("odt", [L.F32, L.BF16])
@pytest.mark.parametrize("per", PER)
def test_random_start_l2_against_fp64(per, odt):
    base = inputs(per, L.F32, L.PGD_BALL_L2)[2]
    b64 = np64(base)
    for box in (None, BOX):
        for valid in (None, ragged_valid(per)):
            got_d, got_o = run_start(per, B, 2, 77, EPS_L2, L.PGD_BALL_L2, base, box, valid, odt)
            ref = R.random_start(B, per, 2, 77, EPS_L2, R.BALL_L2, base=b64, box=box, valid=valid, bf16_operand=odt == L.BF16)
            gd, go, m = np64(got_d), np64(got_o), ref["mask"]
            dev_d, dev_o = np.abs(gd - ref["delta"]), np.abs(go - ref["x"])
            what = f"start_l2/{per}/o{'bf16' if odt else 'f32'}/box{int(box is not None)}/valid{int(valid is not None)}"
            nrm = np.sqrt((gd * gd).sum(axis=1)) / ref["eps"]
            PARITY[what] = {"delta_dev_over_allowed": float((dev_d / np.maximum(ref["allowed_delta"], 1e-300))[m].max(initial=0.0)),
                            "operand_dev_over_allowed": float((dev_o / np.maximum(ref["allowed_x"], 1e-300))[m].max(initial=0.0)),
                            "l2_norm_over_eps": [float(v) for v in nrm]}
            print(what, PARITY[what])
            assert (dev_d <= ref["allowed_delta"]).all() and (dev_o <= ref["allowed_x"]).all(), what
            assert (gd[~m] == 0).all() and torch.equal(bits(got_o)[torch.from_numpy(~m).to(DEV)], bits(base.to(tdt(odt)).to(DEV))[torch.from_numpy(~m).to(DEV)])
            if box is None:                                                                                    # a point ON the sphere
                nv = np.array([per] * B if valid is None else valid)
                assert (np.abs(nrm[nv > 0] - 1) <= 2.0 ** -22).all() and (nrm[nv == 0] == 0).all(), (what, nrm)
            else:
                assert (nrm <= 1 + 2.0 ** -22).all() and (go[m] >= BOX[0]).all() and (go[m] <= BOX[1]).all(), (what, nrm)


@pytest.mark.parametrize("ball", [L.PGD_BALL_LINF, L.PGD_BALL_L2])
@pytest.mark.parametrize("per", [1028, 64 * 1024 + 4])
def test_random_start_half_batches_draw_what_the_whole_batch_draws(per, ball):
    g = torch.Generator(device="cpu").manual_seed(3)
    base = torch.rand(4, per, generator=g) * 2 - 1
    eps = EPS_LINF if ball == L.PGD_BALL_LINF else EPS_L2
    whole_d, whole_o = run_start(per, 4, 0, 99, eps, ball, base, BOX, None, L.BF16)
    for s0 in (0, 2):
        d, o = run_start(per, 2, s0, 99, eps, ball, base[s0:s0 + 2].contiguous(), BOX, None, L.BF16)
        assert torch.equal(bits(d), bits(whole_d[s0:s0 + 2])) and torch.equal(bits(o), bits(whole_o[s0:s0 + 2]))


# ------------------------------------------------------------------------------------------ keep_worst
@pytest.mark.parametrize("odt", [L.F32, L.BF16])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("per", [4, 3072, 64 * 1024 + 4])
def test_keep_worst(per, G, odt):
    D = 5
    nan = float("nan")
    rows = D * G
    stride = 10                                                               # a column of a task's rows [D, 10]
    scores = [[1.0, nan, 3.0, 2.0, -1.0], [1.0, 5.0, nan, 2.5, -0.5], [0.5, 6.0, 4.0, 2.5, nan]]
    bs, bsbuf, bspat = guarded(torch.full((D,), 123.0))
    br, brbuf, brpat = guarded(torch.full((D,), 9, dtype=torch.int32))
    bd, bdbuf, bdpat = guarded(torch.full((rows, per), -7.0))
    bo, bobuf, bopat = guarded(torch.full((rows, per), -7.0).to(tdt(odt)))
    ref = (bs.cpu().numpy(), br.cpu().numpy(), bd.cpu().numpy(), bo.float().cpu().numpy())
    expect_restart = [[0] * 5, [0, 0, 0, 1, 1], [0, 0, 2, 1, 1]]             # ties and NaNs never take after restart 0
    for r, sc in enumerate(scores):
        table = torch.full((D, stride), 1.0e9)
        table[:, 1] = torch.tensor(sc)
        td, tbuf, tpat = guarded(table)
        delta = cpu_randn(rows, per, seed=100 + r)
        op = cpu_randn(rows, per, seed=200 + r).to(tdt(odt))
        dd, dbuf, dpat = guarded(delta)
        od, obuf, opat = guarded(op)
        before_d, before_o = bd.clone(), bo.clone()
        check(lib.rmcl_pgd_keep_worst(P(td[:, 1]), I64(stride), P(bs), P(br), r, D, G, P(dd), P(bd), P(od), P(bo), odt, I64(per), stream()), "pgd_keep_worst")
        torch.cuda.synchronize()
        for buf, pat in ((bsbuf, bspat), (brbuf, brpat), (bdbuf, bdpat), (bobuf, bopat), (tbuf, tpat), (dbuf, dpat), (obuf, opat)):
            assert guards_intact(buf, pat)
        ref = R.keep_worst(sc, ref[0], ref[1], r, G, delta.numpy(), ref[2], op.float().numpy(), ref[3])
        take = ref[4]
        assert br.cpu().tolist() == expect_restart[r] == ref[1].tolist()                            # best_restart is exact
        assert np.array_equal(bs.cpu().numpy().view(np.uint32), ref[0].view(np.uint32))             # NaN bits included
        assert np.array_equal(bd.cpu().numpy(), ref[2]) and np.array_equal(bo.float().cpu().numpy(), ref[3])
        keep_rows = torch.from_numpy(np.repeat(~take, G)).to(DEV)
        assert torch.equal(bits(bd)[keep_rows], bits(before_d)[keep_rows]) and torch.equal(bits(bo)[keep_rows], bits(before_o)[keep_rows])
        if r == 0:
            assert take.all() and torch.isnan(bs[1])                                                # restart 0 takes everything, a NaN score too


# ------------------------------------------------------------------------------------------ rejected calls
def rejected(rc, word):
    assert rc == -1, rc
    assert word.encode() in lib.rmcl_last_error(), lib.rmcl_last_error()


def test_rejected_calls():
    """one call per RMCL_REQUIRE of the three entry points; nothing is launched"""
    t = torch.zeros(B, 8, device=DEV)
    t2 = torch.zeros(B, 8, device=DEV)
    sc = torch.zeros(scratch_bytes(), dtype=torch.uint8, device=DEV)
    i32 = torch.zeros(B, dtype=torch.int32, device=DEV)
    s = stream()

    def step(grad=t, dt=L.F32, delta=t2, scratch=sc, per=8, direction=0, ball=0, lo=0.0, hi=0.0, base=t, op=t, odt=L.F32, flags=0):
        return lib.rmcl_pgd_step_ball(P(grad), dt, P(delta), P(scratch), None, B, I64(per), F(0.1), F(0.1), direction, ball, F(lo), F(hi), P(base), P(op),
                                      odt, flags, s)
    for kw in (dict(grad=None), dict(delta=None), dict(scratch=None)):
        rejected(step(**kw), "NULL")
    rejected(step(per=6), "per_sample")
    rejected(step(dt=2), "dtype")
    rejected(step(odt=7), "dtype")
    rejected(step(direction=3), "direction")
    rejected(step(ball=2), "ball")
    rejected(step(flags=L.PGD_SUM_PREV), "flag")
    rejected(step(base=None), "base")
    rejected(step(base=None, op=None, lo=-1.0, hi=1.0), "base")
    assert step(base=None, op=None) == 0                                       # neither operand nor box: no base needed

    def start(delta=t, scratch=sc, per=8, sample0=0, ball=0, lo=0.0, hi=0.0, base=t, op=t, odt=L.F32):
        return lib.rmcl_pgd_random_start(P(delta), P(scratch), None, B, I64(per), sample0, 1, F(0.1), ball, F(lo), F(hi), P(base), P(op), odt, s)
    rejected(start(delta=None), "NULL")
    rejected(start(scratch=None), "NULL")
    rejected(start(per=10), "per_sample")
    rejected(start(sample0=-1), "sample0")
    rejected(start(odt=5), "dtype")
    rejected(start(ball=-1), "ball")
    rejected(start(base=None), "base")
    rejected(start(base=None, op=None, lo=-1.0, hi=1.0), "base")

    def keep(score=t, stride=1, bs=t, br=i32, r=0, D=B, G=1, delta=t, bd=t, op=t, bo=t, odt=L.F32, per=8):
        return lib.rmcl_pgd_keep_worst(P(score), I64(stride), P(bs), P(br), r, D, G, P(delta), P(bd), P(op), P(bo), odt, I64(per), s)
    for kw in (dict(score=None), dict(bs=None), dict(br=None), dict(delta=None), dict(bd=None), dict(bo=None), dict(op=None)):
        rejected(keep(**kw), "NULL")
    rejected(keep(per=2), "per_sample")
    rejected(keep(G=3), "rows_per_decision")
    rejected(keep(G=0), "rows_per_decision")
    rejected(keep(r=-1), "restart")
    rejected(keep(stride=0), "score_stride")
    rejected(keep(odt=3), "dtype")
    assert int(lib.rmcl_pgd_ball_scratch_bytes(-1)) == -1
    torch.cuda.synchronize()
