"""-m gpu: kernel-level parity of the word-patch-alignment chain of compute_itm_wpa (vilt/modules/objectives.py), the ITM head and the
arena kernels, each through the C ABI against a plain torch float64 reference of the same operation.

Tolerances.  Exact-f32 kernels: 1e-5 relative to the largest magnitude of the reference (fp32 summation order only, the convention of
tests/test_kernels_gpu.py); where a result is a difference of larger terms the scale is the size of those terms, and the test says so.
IPOT: nobody fixed a bound beforehand, so it is derived in the test from the fp32 CPU oracle's own deviation from the fp64 oracle:
e32 = max|O.ipot(float32) - O.ipot(float64)| on the same inputs, allowed = 8 * max(e32, 2^-23 * max T) (the factor covers another
summation order over up to 545 terms and expf against libm, compounded through 50 iterations).  Measured deviations are collected in
PARITY and written as JSON to the file named by RMCL_WPA_PARITY_OUT when that is set (profiles/wpa_kernel_parity.json is such a dump)."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream, gemm, tdt  # noqa: E402
from oracle import rmcl_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
IPOT_FACTOR = 8.0
PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_WPA_PARITY_OUT")
    if out and PARITY:
        with open(out, "w") as f:
            json.dump({"ipot_factor": IPOT_FACTOR, "cases": PARITY}, f, indent=1, sort_keys=True)


def cpu_randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def assert_close(got, ref, tol=TOL, scale=None, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max()) if scale is None else float(scale)
    err = float((got - ref).abs().max())
    print(f"{what}: max |err| {err:.3e}  scale {scale:.3e}  allowed {tol * scale:.3e}")
    assert err <= tol * scale, (what, err, scale)
    return err


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------ 1. row L2 normalise
def l2_inputs(rows, D, eps, seed):
    """A list of [rows, D] inputs.  rows >= 4: one tensor holding an all-zero row, a row whose norm is below eps and a row with a
    50 sigma offset next to ordinary rows; rows == 1: one tensor per kind."""
    tiny = eps * 1e-2 / math.sqrt(D)
    if rows >= 4:
        x = cpu_randn(rows, D, seed=seed)
        x[1] = 0
        x[2] *= tiny
        x[3] += 50
        return [x]
    x = cpu_randn(rows, D, seed=seed)
    return [x, torch.zeros(rows, D), x * tiny, x + 50]


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("rows", [1, 37, 185 * 4])
@pytest.mark.parametrize("D", [768, 64, 100, 1])
def test_l2norm_rows_fwd_bwd(D, rows, eps):
    eps32 = float(torch.tensor(eps, dtype=torch.float32))                       # the value the kernel receives
    for i, x in enumerate(l2_inputs(rows, D, eps, seed=100 + D + rows)):
        xd = x.to(DEV)
        y, nrm = torch.full((rows, D), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
        check(lib.rmcl_l2norm_rows_fwd(P(xd), P(y), P(nrm), rows, D, F(eps), stream()), "l2norm_rows_fwd")
        x64 = x.double()
        n64 = x64.norm(dim=1)
        clamped = n64 < eps32
        nref = n64.clamp_min(eps32)
        yref = x64 / nref[:, None]                                               # F.normalize / clamp_min: x / eps below eps
        yk, nk = y.double().cpu(), nrm.double().cpu()
        assert torch.isfinite(yk).all() and torch.isfinite(nk).all()
        assert ((yk - yref).abs().amax(1) <= TOL * yref.abs().amax(1)).all(), (i, float((yk - yref).abs().max()))
        assert ((nk - nref).abs() <= TOL * nref).all()
        assert (nk[clamped] == eps32).all()
        assert (yk[n64 == 0] == 0).all()

        dy = cpu_randn(rows, D, seed=7 + i)
        dx = torch.full((rows, D), float("nan"), device=DEV)
        dyd = dy.to(DEV)
        check(lib.rmcl_l2norm_rows_bwd(P(dyd), P(y), P(nrm), P(dx), rows, D, stream()), "l2norm_rows_bwd")
        dy64 = dy.double()
        dref = torch.empty(rows, D, dtype=torch.float64)
        if (~clamped).any():                                                     # fp64 autograd of x / max(|x|, eps) above eps
            xa = x64[~clamped].clone().requires_grad_(True)
            (xa / xa.norm(dim=1, keepdim=True).clamp_min(eps32)).backward(dy64[~clamped])
            dref[~clamped] = xa.grad
        # below eps the kernel keeps the unclamped branch: its documented formula (dq - q (q . dq)) / nrm with q = x / eps, nrm = eps
        q = yref[clamped]
        dref[clamped] = (dy64[clamped] - q * (q * dy64[clamped]).sum(1, keepdim=True)) / eps32
        # dx is a difference of terms of size |dq| / nrm (for D = 1 it cancels to zero): the rounding error scales with those terms
        scale = torch.maximum(dref.abs().amax(1), dy64.abs().amax(1) / nref)
        dk = dx.double().cpu()
        assert torch.isfinite(dk).all()
        assert ((dk - dref).abs().amax(1) <= TOL * scale).all(), (i, float(((dk - dref).abs().amax(1) / scale).max()))


# ------------------------------------------------------------------------------------------ 2. the three batched GEMMs
WPA_SHAPES = [(40, 145), (40, 241), (40, 217), (40, 144), (7, 6), (1, 1)]
SENT = -777.25


def unit_rows(n, D, seed):
    return torch.nn.functional.normalize(cpu_randn(n, D, seed=seed), dim=-1)


@pytest.mark.parametrize("nb", [1, 3, 64])
@pytest.mark.parametrize("LtLi", WPA_SHAPES)
def test_gemm_batched_cosine_sim(LtLi, nb):
    """cost[b] = xhat_txt[b] xhat_img[b]^T exactly as compute_itm_wpa issues it: both operands inside ONE [B (Lt + Li), D] buffer,
    C with the padded pitch ld."""
    (Lt, Li), D = LtLi, 768
    N, ld = Lt + Li, (Li + 3) // 4 * 4
    xhat = unit_rows(nb * N, D, seed=Lt + Li + nb).to(DEV)
    cost = torch.full((nb, Lt, ld), SENT, device=DEV)
    check(lib.rmcl_gemm_batched(P(xhat), P(xhat[Lt:]), P(cost), Lt, Li, D, I64(D), I64(D), ld, F(1.0), nb, I64(N * D), I64(N * D),
                                I64(Lt * ld), L.F32, L.F32, 1, 1, stream()), "cosine sim")
    x3 = xhat.double().view(nb, N, D)
    assert_close(cost[:, :, :Li], torch.einsum("bmd,bnd->bmn", x3[:, :Lt], x3[:, Lt:]), what="cosine sim")
    assert (cost[:, :, Li:] == SENT).all()                                       # pad columns of C are not written


@pytest.mark.parametrize("garbage", [False, True])
@pytest.mark.parametrize("nb", [1, 3, 64])
@pytest.mark.parametrize("LtLi", WPA_SHAPES)
def test_gemm_batched_backward_pair(LtLi, nb, garbage):
    """The "d txt" GEMM (reduction over K = Li with lda = ld > K) and the "d img" GEMM (the same operand read transposed).  With
    `garbage` the pad columns Li..ld-1 of that operand hold 1e30: they are outside the problem and must not reach the result."""
    (Lt, Li), D = LtLi, 768
    N, ld = Lt + Li, (Li + 3) // 4 * 4
    xhat = unit_rows(nb * N, D, seed=3 * Lt + Li + nb).to(DEV)
    ds_cpu = cpu_randn(nb, Lt, ld, seed=5 + nb, scale=0.01)
    ds_cpu[:, :, Li:] = 1e30 if garbage else 0.0
    ds = ds_cpu.to(DEV)
    x3, d64 = xhat.double().view(nb, N, D), ds.double()[:, :, :Li]
    dtxt = torch.full((nb * N, D), SENT, device=DEV)
    check(lib.rmcl_gemm_batched(P(ds), P(xhat[Lt:]), P(dtxt), Lt, D, Li, I64(ld), I64(D), D, F(1.0), nb, I64(Lt * ld), I64(N * D),
                                I64(N * D), L.F32, L.F32, 1, 0, stream()), "d txt")
    dtxt = dtxt.view(nb, N, D)
    assert_close(dtxt[:, :Lt], torch.einsum("bmn,bnd->bmd", d64, x3[:, Lt:]), what="d txt")
    assert (dtxt[:, Lt:] == SENT).all()                                          # rows outside [M, N] of C untouched
    dimg = torch.full((nb * N, D), SENT, device=DEV)
    check(lib.rmcl_gemm_batched(P(ds), P(xhat), P(dimg[Lt:]), Li, D, Lt, I64(ld), I64(D), D, F(1.0), nb, I64(Lt * ld), I64(N * D),
                                I64(N * D), L.F32, L.F32, 0, 0, stream()), "d img")
    dimg = dimg.view(nb, N, D)
    assert_close(dimg[:, Lt:], torch.einsum("bmn,bmd->bnd", d64, x3[:, :Lt]), what="d img")
    assert (dimg[:, :Lt] == SENT).all()


@pytest.mark.parametrize("dt", [L.F32, L.BF16])
@pytest.mark.parametrize("K", [145, 41, 3])
@pytest.mark.parametrize("MN", [(37, 50), (130, 131)])
def test_gemm_nt_nn_tn_straddled_vectors(dt, K, MN):
    """Sibling of test_gemm_nt_nn_tn (tests/test_kernels_gpu.py) for the loads that straddle the end of the contiguous dimension: K odd
    and not a multiple of the vector, M and N not multiples of 4 in the M-contiguous layouts, pitches rounded up to the 16-byte vector
    (4 floats / 8 bf16).  The pad elements of BOTH operands hold 1e30, so a tail that is multiplied instead of zeroed overflows."""
    M, N = MN
    V = 4 if dt == L.F32 else 8

    def padded(t):                                                               # [r, c] -> [r, c rounded up to V], pads = 1e30
        out = torch.full((t.shape[0], (t.shape[1] + V - 1) // V * V), 1e30, dtype=t.dtype)
        out[:, :t.shape[1]] = t
        return out.to(DEV)

    X = cpu_randn(M, K, seed=1).to(tdt(dt))
    W = cpu_randn(N, K, seed=2, scale=0.05).to(tdt(dt))
    ref = X.double() @ W.double().t()
    tol = 2e-5 if dt == L.F32 else 1e-2                                          # as test_gemm_nt_nn_tn
    Xp, Wp, Wn, Xt = padded(X), padded(W), padded(W.t()), padded(X.t())
    assert_close(gemm(Xp, Wp, M, N, K, 1, 1, dt, L.F32), ref, tol=tol, what="NT")
    assert_close(gemm(Xp, Wn, M, N, K, 1, 0, dt, L.F32), ref, tol=tol, what="NN")
    assert_close(gemm(Xt, Wn, M, N, K, 0, 0, dt, L.F32), ref, tol=tol, what="TN")


# ------------------------------------------------------------------------------------------ masks shared by 3, 4, 5, 7
def wpa_masks(B, Lt, Li, seed):
    """txt_valid [B, Lt], img_valid [B, Li] int32: random counts (>= 1) at random positions; sample 0 has NO valid text token (an empty
    caption: [CLS][SEP] only, both dropped by the mask), sample 1 every slot valid, sample 2 exactly one valid image slot."""
    assert B >= 3
    g = torch.Generator(device="cpu").manual_seed(seed)
    tl, il = torch.randint(1, Lt + 1, (B,), generator=g), torch.randint(1, Li + 1, (B,), generator=g)
    tl[0], tl[1], il[1], il[2] = 0, Lt, Li, 1
    tv = torch.stack([torch.randperm(Lt, generator=g) < tl[b] for b in range(B)]).to(torch.int32)
    iv = torch.stack([torch.randperm(Li, generator=g) < il[b] for b in range(B)]).to(torch.int32)
    return tv.contiguous(), iv.contiguous()


# ------------------------------------------------------------------------------------------ 3. cost finish
@pytest.mark.parametrize("LtLi", [(40, 145), (40, 241), (40, 144), (7, 6), (1, 1)])
def test_wpa_cost_finish_bitwise(LtLi):
    (Lt, Li), B = LtLi, 5
    ld = (Li + 3) // 4 * 4
    tv, iv = wpa_masks(B, Lt, Li, seed=Lt * Li)
    dots = cpu_randn(B, Lt, ld, seed=11)
    cost = dots.to(DEV)
    tvd, ivd = tv.to(DEV), iv.to(DEV)                                            # (named: a temporary's memory is reused by the next upload)
    check(lib.rmcl_wpa_cost_finish(P(cost), P(tvd), P(ivd), B, Lt, Li, ld, stream()), "cost_finish")
    valid = torch.zeros(B, Lt, ld, dtype=torch.bool)
    valid[:, :, :Li] = (tv[:, :, None] != 0) & (iv[:, None, :] != 0)
    ref = torch.where(valid, 1.0 - dots, torch.zeros(()))
    assert torch.equal(bits(cost), bits(ref))
    assert (cost[:, :, Li:] == 0).all() and (cost[0] == 0).all()


# ------------------------------------------------------------------------------------------ 4. IPOT
def ipot_inputs(B, Lt, Li, family, seed):
    """cost [B, Lt, ld] f32 as the kernel receives it from rmcl_wpa_cost_finish (zero at every masked or pad position) + the masks.
    family "unit": random unit vectors in 768 dimensions, costs ~ 1; "spread": 3-dimensional features, cosines anywhere in [-1, 1]."""
    d = 768 if family == "unit" else 3
    ld = (Li + 3) // 4 * 4
    xt, xi = unit_rows(B * Lt, d, seed=seed).view(B, Lt, d), unit_rows(B * Li, d, seed=seed + 1).view(B, Li, d)
    tv, iv = wpa_masks(B, Lt, Li, seed=seed + 2)
    cost = torch.zeros(B, Lt, ld)
    cost[:, :, :Li] = (1.0 - xt @ xi.transpose(1, 2)).masked_fill((tv[:, :, None] == 0) | (iv[:, None, :] == 0), 0.0)
    return cost, tv, iv


def ipot_oracle(cost, tv, iv, dtype):
    c = cost[:, :, :iv.shape[1]].to(dtype)
    x_pad, y_pad = tv == 0, iv == 0
    return O.ipot(c, tv.sum(1).to(dtype), x_pad, iv.sum(1).to(dtype), y_pad, x_pad[:, :, None] | y_pad[:, None, :], 0.5, 50, 1)


def ipot_kernel(cost, tv, iv):
    B, Lt, ld = cost.shape
    Li = iv.shape[1]
    T = torch.full((B, Li, Lt), SENT, device=DEV)
    costd, tvd, ivd = cost.to(DEV), tv.to(DEV), iv.to(DEV)                       # (named: a temporary's memory is reused by the next upload)
    rc = lib.rmcl_ipot_f32(P(costd), P(tvd), P(ivd), P(T), B, Lt, Li, ld, F(0.5), 50, stream())
    torch.cuda.synchronize()
    return rc, T.cpu()


def ipot_case(Lt, Li, family, B=6, seed=0):
    """Runs one IPOT case, asserts every check of the module docstring and returns the measured figures."""
    cost, tv, iv = ipot_inputs(B, Lt, Li, family, seed=1000 + Lt * Li + seed)
    T64, T32 = ipot_oracle(cost, tv, iv, torch.float64), ipot_oracle(cost, tv, iv, torch.float32)
    assert torch.isfinite(T64).all() and torch.isfinite(T32).all()
    rc, T = ipot_kernel(cost, tv, iv)
    check(rc, "ipot")
    assert torch.isfinite(T).all()
    jp = ((tv[:, :, None] == 0) | (iv[:, None, :] == 0)).transpose(1, 2)         # [B, Li, Lt]
    assert (T[jp] == 0).all() and (T[0] == 0).all()                              # exact zeros at every joint pad; empty caption: T = 0
    live = (tv.sum(1) > 0) & (iv.sum(1) > 0)
    sums = T.double().sum((1, 2))
    # every column of a plan sums to 1 / x_len by construction of the last sigma update; fp32 summation order only
    assert ((sums[live] - 1).abs() <= TOL).all(), sums
    e32 = float((T32.double() - T64).abs().max())
    tmax = float(T64.max())
    base = max(e32, 2.0 ** -23 * tmax)
    dev = float((T.double() - T64).abs().max())
    fig = {"Lt": Lt, "Li": Li, "B": B, "family": family, "max_T": tmax, "e32": e32, "kernel_dev": dev, "allowed": IPOT_FACTOR * base,
           "ratio_to_e32": dev / e32 if e32 > 0 else None, "ratio_to_base": dev / base}
    print("ipot", fig)
    assert dev <= IPOT_FACTOR * base, fig
    return fig


IPOT_BIG = (33, 545)          # largest Li at Lt = 33 under the launcher's 150 KiB rule: (2 * 545 * 34 + 66 + 1090) * 4 = 152 864 bytes of LDS
IPOT_SMALL_SHAPES = [(40, 145), (40, 241), (40, 217), (7, 6), (1, 1)]


def test_ipot_lds_limit_after_a_small_call():
    """The LDS attribute of the kernel is raised lazily and again when a larger problem arrives: small first, then the largest."""
    ipot_case(7, 6, "unit", seed=5)
    PARITY["ipot/lds_limit_after_small"] = ipot_case(*IPOT_BIG, "unit", B=4, seed=5)


def test_ipot_lds_limit_as_first_call_of_a_fresh_process():
    child = ("import json, sys; sys.path.insert(0, sys.argv[1]); from tests.test_wpa_kernels_gpu import ipot_case, IPOT_BIG; "
             "print('IPOT_CHILD ' + json.dumps(ipot_case(*IPOT_BIG, 'spread', B=4, seed=6)))")
    r = subprocess.run([sys.executable, "-c", child, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("IPOT_CHILD ")]
    assert line, r.stdout[-2000:]
    PARITY["ipot/lds_limit_first_call"] = json.loads(line[-1][len("IPOT_CHILD "):])


@pytest.mark.parametrize("family", ["unit", "spread"])
@pytest.mark.parametrize("LtLi", IPOT_SMALL_SHAPES + [IPOT_BIG])
def test_ipot_against_fp64_oracle(LtLi, family):
    PARITY[f"ipot/{LtLi[0]}x{LtLi[1]}/{family}"] = ipot_case(*LtLi, family, B=4 if LtLi == IPOT_BIG else 6)


def test_ipot_rejects_a_problem_beyond_the_lds_rule():
    """(33, 577) needs 161 824 bytes: over the 150 KiB rule.  Non-zero return, a message naming IPOT, nothing launched, and the next
    small call is still right."""
    cost, tv, iv = ipot_inputs(3, 33, 577, "unit", seed=9)
    rc, T = ipot_kernel(cost, tv, iv)
    assert rc != 0
    assert b"ipot" in lib.rmcl_last_error().lower()
    assert (T == SENT).all()
    ipot_case(7, 6, "spread", seed=9)


# ------------------------------------------------------------------------------------------ 5. distance + dsim
@pytest.mark.parametrize("LtLi", [(40, 145), (40, 241), (40, 144), (7, 6), (1, 1)])
def test_wpa_distance_and_dsim(LtLi):
    (Lt, Li), B = LtLi, 5
    ld = (Li + 3) // 4 * 4
    cost_cpu = torch.zeros(B, Lt, ld)
    cost_cpu[:, :, :Li] = cpu_randn(B, Lt, Li, seed=21).abs()
    T_cpu = cpu_randn(B, Li, Lt, seed=22).abs() / (Lt * Li)
    label = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0])
    w_cpu = (2 * label - 1) * 0.1 / B                                            # mixed signs
    cost, T, w = cost_cpu.to(DEV), T_cpu.to(DEV), w_cpu.to(DEV)
    ref = torch.einsum("bmn,bnm->b", cost_cpu[:, :, :Li].double(), T_cpu.double())
    scale = float(torch.einsum("bmn,bnm->b", cost_cpu[:, :, :Li].double().abs(), T_cpu.double().abs()).max())
    dist = torch.full((B,), float("nan"), device=DEV)
    dsim = torch.full((B, Lt, ld), float("nan"), device=DEV)
    check(lib.rmcl_wpa_distance(P(cost), P(T), P(w), P(dist), P(dsim), B, Lt, Li, ld, stream()), "wpa_distance")
    assert_close(dist, ref, scale=scale, what="dist")
    # one fp32 product per element: -w[b] * T[b, n, m] is correctly rounded on both sides
    assert torch.equal(dsim[:, :, :Li].cpu(), (-w_cpu)[:, None, None] * T_cpu.transpose(1, 2))
    assert (dsim[:, :, Li:] == 0).all()                                          # exact zeros (either sign) in the pad columns
    # the inference call: no dsim, no w
    dist2 = torch.full((B,), float("nan"), device=DEV)
    check(lib.rmcl_wpa_distance(P(cost), P(T), None, P(dist2), None, B, Lt, Li, ld, stream()), "wpa_distance (inference)")
    assert torch.equal(dist2, dist)
    assert torch.equal(cost.cpu(), cost_cpu) and torch.equal(T.cpu(), T_cpu)


# ------------------------------------------------------------------------------------------ 6. ITM head
def itm_inputs(B, D, labels, seed):
    cls = cpu_randn(B, D, seed=seed)
    W, bias = cpu_randn(2, D, seed=seed + 1, scale=0.05), cpu_randn(2, seed=seed + 2, scale=0.1)
    dw = W[0] - W[1]
    for b in range(B):                                                           # saturated rows: s0 - s1 ~ +30 / -30
        if b % 4 in (1, 3) or (B == 1 and D == 100):
            cls[b] = (30.0 if b % 4 != 3 else -30.0) * dw / (dw * dw).sum()
    lab = {"zeros": torch.zeros(B), "ones": torch.ones(B), "mixed": (torch.arange(B) % 3 == 0).float()}[labels].to(torch.int32)
    return cls, W, bias, lab


def itm_reference(cls, W, bias, lab, grad_scale):
    logits = cls.double() @ W.double().t() + bias.double()
    loss = (torch.logsumexp(logits, 1) - logits.gather(1, lab.long()[:, None])[:, 0]).mean()
    dl = grad_scale * (torch.softmax(logits, 1) - torch.nn.functional.one_hot(lab.long(), 2).double())
    return logits, loss, dl


@pytest.mark.parametrize("labels", ["zeros", "ones", "mixed"])
@pytest.mark.parametrize("D", [768, 100])
@pytest.mark.parametrize("B", [1, 3, 64, 130])
def test_itm_fwd(B, D, labels):
    cls, W, bias, lab = itm_inputs(B, D, labels, seed=B + D)
    gs = 1.0 / B
    ref_logits, ref_loss, ref_dl = itm_reference(cls, W, bias, lab, gs)
    if B > 1:
        assert float((ref_logits[:, 0] - ref_logits[:, 1]).abs().max()) > 25     # the saturated rows are there
    dev = [t.to(DEV) for t in (cls, W, bias, lab)]
    logits, dlogits = torch.full((B, 2), float("nan"), device=DEV), torch.full((B, 2), float("nan"), device=DEV)
    start = 0.75
    losses = torch.tensor([start, -3.0], device=DEV)
    check(lib.rmcl_itm_fwd(*map(P, dev), P(logits), P(dlogits), P(losses), B, D, F(gs), stream()), "itm_fwd")
    zmax = float(ref_logits.abs().max())
    assert_close(logits, ref_logits, what="logits")
    # loss = lse(z) - z[label] is a difference of terms of size |z|; loss_sum is ADDED to
    assert_close(losses[0], start + ref_loss, scale=max(zmax, start), what="loss_sum")
    assert float(losses[1]) == -3.0
    assert_close(dlogits, ref_dl, scale=gs, what="dlogits")                      # softmax - onehot lies in [-1, 1]
    # loss_sum = NULL and dlogits = NULL are legal
    logits2 = torch.full((B, 2), float("nan"), device=DEV)
    check(lib.rmcl_itm_fwd(*map(P, dev), P(logits2), None, None, B, D, F(gs), stream()), "itm_fwd (no loss, no dlogits)")
    assert torch.equal(logits2, logits)


@pytest.mark.parametrize("labels", ["zeros", "ones", "mixed"])
@pytest.mark.parametrize("D", [768, 100])
@pytest.mark.parametrize("B", [1, 3, 64, 130])
def test_itm_bwd(B, D, labels):
    cls, W, bias, lab = itm_inputs(B, D, labels, seed=B + D)
    _, _, ref_dl = itm_reference(cls, W, bias, lab, 1.0 / B)
    dl = ref_dl.float()                                                          # the kernel's input: the reference dlogits in fp32
    dl64, scale = dl.double(), 0.37
    ref_dcls = scale * dl64 @ W.double()
    term_cls = float((scale * dl64.abs() @ W.double().abs()).max())               # dl[b, 0] = -dl[b, 1]: the two products behind dcls cancel
    ref_dW, ref_db = scale * dl64.t() @ cls.double(), scale * dl64.sum(0)
    term_W = scale * dl64.abs().t() @ cls.double().abs()                         # size of the sums behind dW (they cancel across samples)
    d_dl, d_cls, d_W = dl.to(DEV), cls.to(DEV), W.to(DEV)
    gw0, gb0 = cpu_randn(2, D, seed=77), cpu_randn(2, seed=78)
    gw, gb = gw0.to(DEV), gb0.to(DEV)
    dcls = torch.full((B, D), float("nan"), device=DEV)
    for n in (1, 2):                                                             # dW / db ACCUMULATE: non-zero start, two calls
        check(lib.rmcl_itm_bwd(P(d_dl), P(d_cls), P(d_W), P(dcls), P(gw), P(gb), B, D, F(scale), stream()), "itm_bwd")
        assert_close(dcls, ref_dcls, scale=term_cls, what="dcls")
        assert_close(gw, gw0.double() + n * ref_dW, scale=float((gw0.double().abs() + n * term_W).max()), what=f"dW after {n}")
        assert_close(gb, gb0.double() + n * ref_db, scale=float((gb0.double().abs() + n * scale * dl64.abs().sum(0)).max()),
                     what=f"db after {n}")
    # frozen head (IRTR): dW = db = NULL writes only dcls; scale = 1
    dcls2 = torch.full((B, D), float("nan"), device=DEV)
    check(lib.rmcl_itm_bwd(P(d_dl), P(d_cls), P(d_W), P(dcls2), None, None, B, D, F(1.0), stream()), "itm_bwd (frozen head)")
    assert_close(dcls2, dl64 @ W.double(), scale=term_cls / scale, what="dcls (frozen head)")


# ------------------------------------------------------------------------------------------ 7. the chain
def chain_reference(xn, tv, iv, w, B, Lt, Li, dtype, T_fixed=None):
    """The oracle's formulation (oracle/rmcl_oracle.py compute_itm_wpa): cost through F.normalize(eps = 1e-5), T detached,
    0.1 (sum_pos - sum_neg) / B = sum_b w_b dist_b."""
    D = xn.shape[1]
    x = xn.to(dtype).clone().requires_grad_(True)
    xh = torch.nn.functional.normalize(x.view(B, Lt + Li, D), dim=-1, eps=1e-5)
    x_pad, y_pad = tv == 0, iv == 0
    jp = x_pad[:, :, None] | y_pad[:, None, :]
    cost = (1 - xh[:, :Lt] @ xh[:, Lt:].transpose(1, 2)).masked_fill(jp, 0)
    T = O.ipot(cost.detach(), tv.sum(1).to(dtype), x_pad, iv.sum(1).to(dtype), y_pad, jp, 0.5, 50, 1) if T_fixed is None else T_fixed
    dist = torch.einsum("bmn,bnm->b", cost, T.detach())
    loss = (dist * w.to(dtype)).sum()
    loss.backward()
    return loss.detach(), x.grad, T.detach(), cost.detach(), dist.detach()


@pytest.mark.parametrize("LiB", [(145, 4), (241, 3)])
def test_wpa_chain_loss_and_dxn(LiB):
    """Calls 1-7 of compute_itm_wpa and its four backward calls, as it issues them, against fp64 autograd."""
    (Li, B), Lt, D = LiB, 40, 768
    N, ld = Lt + Li, (Li + 3) // 4 * 4
    M = B * N
    xn_cpu = cpu_randn(M, D, seed=31 + Li)
    tv, iv = wpa_masks(B, Lt, Li, seed=32 + Li)
    label = torch.tensor([1.0, 0.0, 1.0, 0.0][:B])
    w_cpu = (2 * label - 1) * (0.1 / B)
    xn, txt_valid, img_valid, w = xn_cpu.to(DEV), tv.to(DEV), iv.to(DEV), w_cpu.to(DEV)
    st = stream()
    xhat, norms = torch.empty(M, D, device=DEV), torch.empty(M, device=DEV)
    check(lib.rmcl_l2norm_rows_fwd(P(xn), P(xhat), P(norms), M, D, F(1e-5), st), "l2norm")
    cost = torch.zeros(B, Lt, ld, device=DEV)
    check(lib.rmcl_gemm_batched(P(xhat), P(xhat[Lt:]), P(cost), Lt, Li, D, I64(D), I64(D), ld, F(1.0), B, I64(N * D), I64(N * D),
                                I64(Lt * ld), L.F32, L.F32, 1, 1, st), "cosine sim")
    check(lib.rmcl_wpa_cost_finish(P(cost), P(txt_valid), P(img_valid), B, Lt, Li, ld, st), "cost_finish")
    T = torch.empty(B, Li, Lt, device=DEV)
    check(lib.rmcl_ipot_f32(P(cost), P(txt_valid), P(img_valid), P(T), B, Lt, Li, ld, F(0.5), 50, st), "ipot")
    dist, dsim = torch.empty(B, device=DEV), torch.empty(B, Lt, ld, device=DEV)
    check(lib.rmcl_wpa_distance(P(cost), P(T), P(w), P(dist), P(dsim), B, Lt, Li, ld, st), "wpa_distance")
    loss = (dist * w).sum()
    dxhat = torch.zeros(M, D, device=DEV)
    check(lib.rmcl_gemm_batched(P(dsim), P(xhat[Lt:]), P(dxhat), Lt, D, Li, I64(ld), I64(D), D, F(1.0), B, I64(Lt * ld), I64(N * D),
                                I64(N * D), L.F32, L.F32, 1, 0, st), "d txt")
    check(lib.rmcl_gemm_batched(P(dsim), P(xhat), P(dxhat[Lt:]), Li, D, Lt, I64(ld), I64(D), D, F(1.0), B, I64(Lt * ld), I64(N * D),
                                I64(N * D), L.F32, L.F32, 0, 0, st), "d img")
    dxn = torch.empty(M, D, device=DEV)
    check(lib.rmcl_l2norm_rows_bwd(P(dxhat), P(xhat), P(norms), P(dxn), M, D, st), "l2norm_bwd")

    loss64, dxn64, T64, cost64, dist64 = chain_reference(xn_cpu, tv, iv, w_cpu, B, Lt, Li, torch.float64)
    loss32, dxn32, T32, _, _ = chain_reference(xn_cpu, tv, iv, w_cpu, B, Lt, Li, torch.float32)
    Tk = T.double().cpu()
    e32_T = float((T32.double() - T64).abs().max())
    tol_T = IPOT_FACTOR * max(e32_T, 2.0 ** -23 * float(T64.max()))
    dev_T = float((Tk - T64).abs().max())
    # a deviation dT of the plan moves row m of dxhat by w sum_n dT[n, m] xhat_img[n]: at most |w| Li tol_T in 2-norm because every
    # |xhat row| = 1; the projection of the normalise backward does not lengthen it and the division by the row norm shrinks it
    wmax, nmin = float(w_cpu.abs().max()), float(xn_cpu.double().norm(dim=1).min())
    tol_dxn = TOL * float(dxn64.abs().max()) + wmax * max(Lt, Li) * tol_T / nmin
    tol_loss = TOL * float((dist64 * w_cpu.double()).abs().sum()) + float((w_cpu.double().abs() * cost64.sum((1, 2))).sum()) * tol_T
    dev_dxn, dev_loss = float((dxn.double().cpu() - dxn64).abs().max()), abs(float(loss) - float(loss64))
    e32_dxn, e32_loss = float((dxn32.double() - dxn64).abs().max()), abs(float(loss32) - float(loss64))
    fig = {"Lt": Lt, "Li": Li, "B": B, "T": {"e32": e32_T, "kernel_dev": dev_T, "allowed": tol_T, "ratio_to_e32": dev_T / e32_T if e32_T > 0 else None},
           "dxn": {"max_ref": float(dxn64.abs().max()), "e32": e32_dxn, "kernel_dev": dev_dxn, "allowed": tol_dxn,
                   "ratio_to_e32": dev_dxn / e32_dxn if e32_dxn > 0 else None},
           "loss": {"ref": float(loss64), "e32": e32_loss, "kernel_dev": dev_loss, "allowed": tol_loss,
                    "ratio_to_e32": dev_loss / e32_loss if e32_loss > 0 else None}}
    # the same backward with the plan held at the KERNEL's T (T is detached, so it is a constant of the backward): no IPOT term left,
    # the plain 1e-5 of the exact-f32 kernels applies to dxn and to the loss
    loss_f, dxn_f, _, _, dist_f = chain_reference(xn_cpu, tv, iv, w_cpu, B, Lt, Li, torch.float64, T_fixed=Tk)
    dev_dxn_f = float((dxn.double().cpu() - dxn_f).abs().max())
    fig["dxn_at_kernel_T"] = {"max_ref": float(dxn_f.abs().max()), "kernel_dev": dev_dxn_f, "allowed": TOL * float(dxn_f.abs().max())}
    print("chain", fig)
    PARITY[f"chain/{Lt}x{Li}"] = fig
    assert torch.isfinite(dxn).all() and torch.isfinite(T).all()
    assert dev_T <= tol_T, fig
    assert dev_loss <= tol_loss, fig
    assert dev_dxn <= tol_dxn, fig
    assert_close(loss, loss_f, scale=float((dist_f * w_cpu.double()).abs().sum()), what="loss at the kernel's T")
    assert_close(dxn, dxn_f, what="dxn at the kernel's T")


# ------------------------------------------------------------------------------------------ 8. arena kernels
BIG_N = 8192 * 1024 * 4 + 4                                                     # one element group more than the capped grid covers in one pass
INF, NAN = float("inf"), float("nan")
# bf16 ties: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7 (even mantissa below: rounds down), 1 + 3 * 2^-8 rounds up to the even 1 + 2^-6
SPECIAL_A = [INF, NAN, 1.00390625, 1.01171875, -INF, -1.00390625, 1.0, INF, 3.4e38, -1.01171875, 0.0, 255.5]
SPECIAL_D1 = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.00390625, -INF, 0.0, 0.0, -0.0, 0.0]   # a tie that only the SUM produces; inf - inf = NaN


@functools.lru_cache(maxsize=None)
def cast_operands(n):
    a, d1, d2 = cpu_randn(n, seed=41), cpu_randn(n, seed=42, scale=0.03), cpu_randn(n, seed=43, scale=0.03)
    k = min(n, len(SPECIAL_A))
    a[:k], d1[:k], d2[:k] = torch.tensor(SPECIAL_A[:k]), torch.tensor(SPECIAL_D1[:k]), 0.0
    return a, d1, d2


def assert_same_bits(got, ref):
    """Bit equality; a NaN has no unique encoding, so there only NaN-ness is compared."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(bits(got)[~nan.cpu()], bits(ref)[~nan.cpu()])


@pytest.mark.parametrize("dt", [L.F32, L.BF16])
@pytest.mark.parametrize("n", [4, 1028, BIG_N])
def test_cast_f32(n, dt):
    a = cast_operands(n)[0].to(DEV)
    out = torch.zeros(n, dtype=tdt(dt), device=DEV)
    check(lib.rmcl_cast_f32(P(a), P(out), dt, I64(n), stream()), "cast")
    assert_same_bits(out, a.to(tdt(dt)))                                         # torch's cast rounds to nearest even


@pytest.mark.parametrize("with_d2", [False, True])
@pytest.mark.parametrize("with_d1", [False, True])
@pytest.mark.parametrize("dt", [L.F32, L.BF16])
@pytest.mark.parametrize("n", [4, 1028, BIG_N])
def test_add_cast_f32(n, dt, with_d1, with_d2):
    a, d1, d2 = (t.to(DEV) for t in cast_operands(n))
    d1, d2 = (d1 if with_d1 else None), (d2 if with_d2 else None)
    out = torch.zeros(n, dtype=tdt(dt), device=DEV)
    check(lib.rmcl_add_cast_f32(P(a), P(d1), P(d2), P(out), dt, I64(n), stream()), "add_cast")
    s = a
    if d1 is not None:
        s = s + d1
    if d2 is not None:
        s = s + d2                                                               # (a + d1) + d2 in fp32
    assert_same_bits(out, s.to(tdt(dt)))


def test_cast_rejects_n_not_a_multiple_of_4():
    a, out = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    assert lib.rmcl_cast_f32(P(a), P(out), L.F32, I64(6), stream()) != 0
    assert lib.rmcl_add_cast_f32(P(a), P(a), None, P(out), L.BF16, I64(6), stream()) != 0
    assert b"add_cast" in lib.rmcl_last_error()


@pytest.mark.parametrize("pp", [1024, 4])
@pytest.mark.parametrize("rows", [1, 144 * 4, 144 * 64])
def test_delta_channel_norm(rows, pp):
    Cc = 3
    delta = cpu_randn(rows, Cc * pp, seed=51, scale=0.03)
    start = 12.5
    out = torch.tensor([start], device=DEV)
    deltad = delta.to(DEV)
    check(lib.rmcl_delta_channel_norm(P(deltad), P(out), I64(rows), Cc, pp, stream()), "delta_channel_norm")
    ref = delta.double().view(rows, Cc, pp).pow(2).sum(1).sqrt().sum() + start  # out is ADDED to
    assert_close(out[0], ref, what="delta_channel_norm")


def test_delta_channel_norm_rejects_pp_not_a_multiple_of_4():
    delta, out = torch.zeros(64, device=DEV), torch.zeros(1, device=DEV)
    assert lib.rmcl_delta_channel_norm(P(delta), P(out), I64(1), 3, 6, stream()) != 0
    assert b"delta_chan_norm" in lib.rmcl_last_error()
    torch.cuda.synchronize()
    assert float(out) == 0.0


@functools.lru_cache(maxsize=None)
def arena():
    d = L.Dims(B=2, L=40, P=144, D=768, H=12, layers=2, mlp=3072, patch_k=3072, proj=128, vocab=30522, dtype=L.BF16, exact=0, Pp=144)
    lay = L.Layout()
    lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    return d, lay, cpu_randn(lay.total, seed=61, scale=0.5)                      # random gamma, beta, W, b everywhere


def test_ln_fold():
    d, lay, p32 = arena()
    D, mlp, layers = d.D, d.mlp, d.layers
    rows = 3 * D + mlp
    nw, ns = lib.rmcl_ln_fold_elems(C.byref(d), 0), lib.rmcl_ln_fold_elems(C.byref(d), 1)
    assert nw == layers * rows * D and ns == layers * 2 * rows
    wf, sc = torch.zeros(nw, dtype=torch.bfloat16, device=DEV), torch.full((ns,), float("nan"), device=DEV)
    p32d = p32.to(DEV)
    check(lib.rmcl_ln_fold(C.byref(d), P(p32d), P(wf), P(sc), stream()), "ln_fold")
    wf, sc = wf.cpu().view(layers, rows, D), sc.double().cpu().view(layers, 2, rows)
    for l in range(layers):
        base = lay.layer0 + l * lay.layer_stride
        for w_off, b_off, g_off, be_off, n, r0 in ((lay.qkv_w, lay.qkv_b, lay.ln1_w, lay.ln1_b, 3 * D, 0),
                                                   (lay.fc1_w, lay.fc1_b, lay.ln2_w, lay.ln2_b, mlp, 3 * D)):
            W = p32[base + w_off:base + w_off + n * D].view(n, D)
            gam, bet, bias = p32[base + g_off:base + g_off + D], p32[base + be_off:base + be_off + D], p32[base + b_off:base + b_off + n]
            w_ref = (W * gam).to(torch.bfloat16)                                 # bf16(fp32(W gamma))
            assert torch.equal(bits(wf[l, r0:r0 + n]), bits(w_ref))
            # s = row sums of the ROUNDED wf (what the matrix cores multiply by), c = W beta + b
            s_terms, c_terms = w_ref.double(), W.double() * bet.double()
            assert ((sc[l, 0, r0:r0 + n] - s_terms.sum(1)).abs() <= TOL * s_terms.abs().sum(1)).all()
            assert ((sc[l, 1, r0:r0 + n] - (c_terms.sum(1) + bias.double())).abs() <= TOL * (c_terms.abs().sum(1) + bias.double().abs())).all()


def test_weight_transpose_bf16():
    d, lay, p32 = arena()
    src = p32.to(torch.bfloat16)
    expect = torch.full((lay.total,), -3.0, dtype=torch.bfloat16)               # everything else in the destination stays as it was
    dst = expect.to(DEV)
    for l in range(d.layers):
        base = lay.layer0 + l * lay.layer_stride
        for off, r, c in ((lay.qkv_w, 3 * d.D, d.D), (lay.proj_w, d.D, d.D), (lay.fc1_w, d.mlp, d.D), (lay.fc2_w, d.D, d.mlp)):
            expect[base + off:base + off + r * c] = src[base + off:base + off + r * c].view(r, c).t().reshape(-1)
    srcd = src.to(DEV)
    check(lib.rmcl_weight_transpose_bf16(C.byref(d), P(srcd), P(dst), stream()), "weight_transpose")
    assert torch.equal(bits(dst), bits(expect))
