"""-m gpu: rmcl_ipot_plan_f32 and rmcl_align_heat (csrc/align.hip) through the C ABI.

IPOT.  Against oracle.rmcl_oracle.ipot in float64 under the rule of tests/test_wpa_kernels_gpu.py: e32 = max |O.ipot(f32) - O.ipot(f64)|
on the same inputs, allowed = 8 * max(e32, 2^-23 max T).  The factor 8 is that module's; it covered another summation order compounded
over 50 iterations, and the 1000-iteration cases here are held to it unchanged.  A case whose allowance exceeds 1e-3 max T is an INPUT
failure (the fp32 oracle itself is lost there - the degenerate `spread` problem at (7, 6)) and fails the test.  Every kernel_dev / base
ratio is collected in PARITY and written as JSON to the file named by RMCL_ALIGN_PARITY_OUT when that is set
(profiles/align_parity.json is such a dump).  Exact checks: zeros at every joint pad, plan sums within 1e-5 of 1, a sentinel-filled
output fully overwritten, identical bytes on a second call; agreement with rmcl_ipot_f32 at (beta 0.5, 50 iterations) within the same
allowance wherever that kernel's LDS rule takes the shape.

Heat.  The fp32 plan is fed to the kernel and to the float64 model of tests/align_ref.py, so the kernel is judged alone: grid bit-equal to
the scatter, heat within align_ref.heat_allowance (the kernel's fp64 accumulation, one rounding to fp32), flat equal, alpha byte-equal
with no exemption - the input generator refuses a seed in which some 255 * heat of the float64 model lies within 255 * allowance of an
integer other than at exactly 0 and 255.  Guard words surround every output."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, lib, check, P, F, stream  # noqa: E402
from oracle import rmcl_oracle as O  # noqa: E402
from tests import align_ref as R  # noqa: E402
from tests.test_wpa_kernels_gpu import ipot_inputs, IPOT_FACTOR, SENT  # noqa: E402

PARITY = {}
MEANINGFUL = 1e-3
LTS = [1, 7, 39, 40]
LIS = [1, 2, 63, 64, 65, 145, 255, 256, 257, 472, 512]      # both sides of the wave and of the one-row / two-row boundary
LONG = [(40, 145), (40, 257), (40, 472), (40, 512), (39, 256), (7, 65), (40, 64), (1, 145), (40, 255), (7, 472)]
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_ALIGN_PARITY_OUT")
    if out and PARITY:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec["kernels"] = {"ipot_factor": IPOT_FACTOR, "what": "rmcl_ipot_plan_f32 against O.ipot(float64): kernel_dev / base, base = max(e32, 2^-23 max T), "
                          "allowed ratio = ipot_factor; rmcl_align_heat: largest |heat - model| / allowance", "cases": PARITY}
        with open(out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")


def oracle(cost, tv, iv, dtype, beta, iters):
    c = cost[:, :, :iv.shape[1]].to(dtype)
    x_pad, y_pad = tv == 0, iv == 0
    with np.errstate(all="ignore"):
        return O.ipot(c, tv.sum(1).to(dtype), x_pad, iv.sum(1).to(dtype), y_pad, x_pad[:, :, None] | y_pad[:, None, :], beta, iters, 1)


def plan_kernel(cost, tv, iv, beta, iters, Lt=None, Li=None, which="plan"):
    B, Lt0, ld = cost.shape
    Lt, Li = Lt0 if Lt is None else Lt, iv.shape[1] if Li is None else Li
    T = torch.full((B, iv.shape[1], Lt0), SENT, device=DEV)
    costd, tvd, ivd = cost.to(DEV), tv.to(DEV), iv.to(DEV)                       # (named: a temporary's memory is reused by the next upload)
    fn = lib.rmcl_ipot_plan_f32 if which == "plan" else lib.rmcl_ipot_f32
    rc = fn(P(costd), P(tvd), P(ivd), P(T), B, Lt, Li, ld, F(beta), iters, stream())
    torch.cuda.synchronize()
    return rc, T.cpu()


def old_kernel_takes(Lt, Li):
    return (2 * Li * (Lt + 1) + 2 * Lt + 2 * Li) * 4 <= 150 * 1024              # csrc/ipot.hip: the LDS rule of rmcl_ipot_f32


def plan_case(Lt, Li, family, B, beta, iters, seed=0):
    cost, tv, iv = ipot_inputs(B, Lt, Li, family, seed=2000 + Lt * Li + seed)
    T64, T32 = oracle(cost, tv, iv, torch.float64, beta, iters), oracle(cost, tv, iv, torch.float32, beta, iters)
    assert torch.isfinite(T64).all() and torch.isfinite(T32).all()
    rc, T = plan_kernel(cost, tv, iv, beta, iters)
    check(rc, "ipot_plan")
    assert torch.isfinite(T).all() and not (T == SENT).any()                     # the sentinel-filled output is fully overwritten
    jp = ((tv[:, :, None] == 0) | (iv[:, None, :] == 0)).transpose(1, 2)         # [B, Li, Lt]
    assert (T[jp] == 0).all() and (T[0] == 0).all()                              # exact zeros at every joint pad; empty caption: T = 0
    live = (tv.sum(1) > 0) & (iv.sum(1) > 0)
    assert ((T.double().sum((1, 2))[live] - 1).abs() <= 1e-5).all()
    rc2, T2 = plan_kernel(cost, tv, iv, beta, iters)
    assert rc2 == 0 and torch.equal(T.view(torch.int32), T2.view(torch.int32))   # identical bytes on a second call
    e32, tmax = float((T32.double() - T64).abs().max()), float(T64.max())
    base = max(e32, 2.0 ** -23 * tmax)
    allowed = IPOT_FACTOR * base
    dev = float((T.double() - T64).abs().max())
    fig = {"Lt": Lt, "Li": Li, "B": B, "family": family, "beta": beta, "iters": iters, "max_T": tmax, "e32": e32, "kernel_dev": dev,
           "allowed": allowed, "ratio_to_base": dev / base}
    if beta == 0.5 and iters == 50 and old_kernel_takes(Lt, Li):
        rc3, Told = plan_kernel(cost, tv, iv, beta, iters, which="old")
        check(rc3, "ipot")
        fig["dev_from_rmcl_ipot_f32"] = float((T.double() - Told.double()).abs().max())
    print("ipot_plan", fig)
    assert allowed <= MEANINGFUL * tmax, ("input failure: the fp32 oracle itself is lost on this problem", fig)
    assert dev <= allowed, fig
    assert fig.get("dev_from_rmcl_ipot_f32", 0.0) <= allowed, fig
    return fig


@pytest.mark.parametrize("B", [3, 6])
@pytest.mark.parametrize("Li", LIS)
@pytest.mark.parametrize("Lt", LTS)
def test_ipot_plan_against_fp64_oracle(Lt, Li, B):
    for iters in (1, 50):
        PARITY[f"ipot_plan/{Lt}x{Li}/B{B}/unit/i{iters}"] = plan_case(Lt, Li, "unit", B, 0.5, iters)


@pytest.mark.parametrize("Li", [145, 257, 472])
def test_ipot_plan_spread_family(Li):
    for iters in (1, 50):
        PARITY[f"ipot_plan/40x{Li}/B3/spread/i{iters}"] = plan_case(40, Li, "spread", 3, 0.5, iters, seed=1)


@pytest.mark.parametrize("LtLi", LONG)
def test_ipot_plan_1000_iterations_at_beta_01(LtLi):
    PARITY[f"ipot_plan/{LtLi[0]}x{LtLi[1]}/B3/unit/i1000"] = plan_case(*LtLi, "unit", 3, 0.1, 1000, seed=2)


def test_ipot_plan_rejects_calls_beyond_its_limits():
    """Lt = 41, Li = 513, iters = 0 / 10001, beta = 0: non-zero, a message naming the limit, nothing launched (the sentinel stays), and a
    following small call is right."""
    # buffers larger than any shape asked for below: a call that got past its check would still stay inside them
    cost, tv, iv = torch.zeros(3, 41, 516), torch.ones(3, 41, dtype=torch.int32), torch.ones(3, 513, dtype=torch.int32)
    for kw, word in ((dict(Lt=41), b"Lt"), (dict(Li=513), b"Li"), (dict(iters=0), b"iters"), (dict(iters=10001), b"iters"),
                     (dict(beta=0.0), b"beta"), (dict(beta=-0.5), b"beta")):
        a = dict(Lt=40, Li=512, beta=0.5, iters=50)
        a.update(kw)
        rc, T = plan_kernel(cost, tv, iv, a["beta"], a["iters"], Lt=a["Lt"], Li=a["Li"])
        assert rc != 0, kw
        msg = lib.rmcl_last_error()
        assert b"ipot_plan" in msg and word in msg, (kw, msg)
        assert (T == SENT).all(), kw
    plan_case(7, 6, "unit", 3, 0.5, 50, seed=9)


# ------------------------------------------------------------------------------------------ heat maps
def guarded(shape, dtype, fill):
    """(view of `shape` inside a buffer with GUARD sentinel elements on both sides, the buffer)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def heat_inputs(B, Lt, H, W, seed):
    """plan [B, Li, Lt] fp32 (peaked, non-negative; sample 0 keeps every patch and has a constant and an all-zero column; the other samples
    keep a random subset in row-major order and have padding slots), patch_index, txt_valid (position 0 of every sample and one more are
    masked), one token per sample; the seed is advanced until the float64 model has the byte margin of the module docstring."""
    HW = H * W
    for s in range(seed, seed + 50):
        rng = np.random.RandomState(s)
        P_ = HW
        T = (rng.rand(B, P_ + 1, Lt) ** 8).astype(np.float32)
        pidx = np.full((B, P_), -1, dtype=np.int32)
        pidx[0] = np.arange(HW)
        for b in range(1, B):
            k = max(1, int(rng.randint(HW // 2, HW + 1)))
            pidx[b, :k] = np.sort(rng.permutation(HW)[:k])
            T[b, 1 + k:] = 0                                                      # padding slots carry no mass
        if Lt > 3:
            T[0, :, 2], T[0, :, 3] = 0.25, 0.0
        tv = np.ones((B, Lt), dtype=np.int32)
        tv[:, 0] = 0
        if Lt > 1:
            tv[np.arange(B), rng.randint(1, Lt, size=B)] = 0
        grid = R.scatter(T, pidx, H, W)
        heat, flat = R.heat_model(grid, tv)
        good = True
        for b, m in zip(*np.nonzero(flat == 0)):
            if (R.byte_margin(heat[b, m]) <= 255.0 * R.heat_allowance(grid[b, m])).any():
                good = False
        if good:
            token = [int(np.flatnonzero(flat[b] == 0)[0]) if (flat[b] == 0).any() else 0 for b in range(B)]
            if B > 1:
                token[1] = 0                                                      # a flat (masked) position: its alpha is all zero
            return T, pidx, tv, token, grid, heat, flat
    raise AssertionError("no seed with the byte margin")


@pytest.mark.parametrize("HW,size", [((1, 1), (5, 7)), ((1, 2), (4, 9)), ((3, 4), (96, 128)), ((12, 20), (333, 500)), ((12, 20), (5, 7))])
def test_align_heat_against_the_float64_model(HW, size):
    (H, W), (Ho, Wo), B, Lt = HW, size, 3, 6
    T, pidx, tv, token, grid64, heat64, flat64 = heat_inputs(B, Lt, H, W, seed=10 * H + W)
    Li = T.shape[1]
    Td, pd_, tvd = torch.from_numpy(T).to(DEV), torch.from_numpy(pidx).to(DEV), torch.from_numpy(tv).to(DEV)
    tables = torch.tensor(R.nearest_table(H, Ho).tolist() + R.nearest_table(W, Wo).tolist(), dtype=torch.int32, device=DEV)
    tok = torch.tensor(token, dtype=torch.int32, device=DEV)
    grid, gbuf = guarded((B, Lt, H, W), torch.float32, SENT)
    heat, hbuf = guarded((B, Lt, H, W), torch.float32, SENT)
    flat, fbuf = guarded((B, Lt), torch.int32, -7)
    alpha, abuf = guarded((B, Ho, Wo), torch.uint8, 0x5A)
    check(lib.rmcl_align_heat(P(Td), P(pd_), P(tvd), B, Lt, Li, H, W, P(grid), P(heat), P(flat), P(tok), P(tables), Ho, Wo, P(alpha),
                              stream()), "align_heat")
    torch.cuda.synchronize()
    assert guards_intact(gbuf, SENT) and guards_intact(hbuf, SENT) and guards_intact(fbuf, -7) and guards_intact(abuf, 0x5A)
    want_grid = R.scatter(T, pidx, H, W)
    assert np.array_equal(grid.cpu().numpy().view(np.int32), want_grid.view(np.int32))       # bit-equal to the scatter
    assert np.array_equal(flat.cpu().numpy(), flat64)
    assert flat64[:, 0].all() and (H * W >= 12) == bool((flat64 == 0).any())                # masked positions; tiny grids are flat
    hk = heat.cpu().numpy().astype(np.float64)
    assert np.isfinite(hk).all() and (hk[flat64 == 1] == 0).all()
    worst = 0.0
    for b, m in zip(*np.nonzero(flat64 == 0)):
        allow = R.heat_allowance(grid64[b, m])
        err = float(np.abs(hk[b, m] - heat64[b, m]).max())
        worst = max(worst, err / allow)
        assert err <= allow, (b, m, err, allow)
    PARITY[f"align_heat/{H}x{W}"] = {"largest_error_over_allowance": worst}
    for b in range(B):
        assert np.array_equal(alpha[b].cpu().numpy(), R.alpha_bytes(heat64[b, token[b]], Ho, Wo)), b
    if B > 1:
        assert not alpha[1].any()
    # without alpha: token / tables are not read, and the other outputs are the same bytes
    grid2, heat2, flat2 = torch.empty_like(grid), torch.empty_like(heat), torch.empty_like(flat)
    check(lib.rmcl_align_heat(P(Td), P(pd_), P(tvd), B, Lt, Li, H, W, P(grid2), P(heat2), P(flat2), None, None, 0, 0, None, stream()), "align_heat")
    assert torch.equal(grid2, grid) and torch.equal(heat2.view(torch.int32), heat.view(torch.int32)) and torch.equal(flat2, flat)


def test_align_heat_rejects_bad_arguments():
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    a = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert lib.rmcl_align_heat(None, P(i), P(i), 1, 2, 3, 1, 2, P(t), P(t), P(i), None, None, 0, 0, None, stream()) == -1
    assert b"align_heat" in lib.rmcl_last_error() and b"NULL" in lib.rmcl_last_error()
    assert lib.rmcl_align_heat(P(t), P(i), P(i), 1, 2, 3, 65, 64, P(t), P(t), P(i), None, None, 0, 0, None, stream()) == -1
    assert b"4096" in lib.rmcl_last_error()
    assert lib.rmcl_align_heat(P(t), P(i), P(i), 1, 2, 3, 1, 2, P(t), P(t), P(i), None, P(i), 2, 2, P(a), stream()) == -1
    assert b"token" in lib.rmcl_last_error()
