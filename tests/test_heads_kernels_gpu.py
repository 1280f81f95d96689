"""-m gpu: rmcl_heads_forward / rmcl_heads_forward2 / rmcl_heads_backward (pooler, MoCo projector, L2 normalise) called by name and
compared with float64 autograd at the batch sizes where the host-side chain of csrc/api.cpp picks other kernels: the skinny pooler GEMM
with the duplicated cls_feats output up to B = 1024 and the general kernel + copy beyond, the short-K weight-gradient kernel with its
column-sum by-product up to B = 256 and the separate column sum beyond (or at any B with rmcl_tune_set(6, 0)), the in-place strided read
of RMCL_HEADS_NO_WGRAD, every combination of dq / dcls_extra / grads32.

Reference (operation order of heads.py Pooler / MocoHead and objectives.py:264-269 of the reference project):
  pooled = tanh(xn[:, 0] Wp^T + bp); h1 = pooled W0^T + b0; h2 = relu(LN(h1; g, b, eps 1e-5)); z = h2 W3^T; q = z / max(|z|, 1e-12)
in float64 on the fp32 values the kernels read; gradients by autograd of sum(q * dq) + sum(pooled * dcls_extra).  Rows 1..N-1 of every
sample of xn hold 1e30: only row 0 may be read.  The stash and the scratch rows start as NaN: nothing stale may be read either.

ReLU kink.  A pre-ReLU value within fp32 rounding of zero may take the other branch on the device, which moves a gradient by O(1) without
being an error.  Rows of the float64 forward with a pre-ReLU element below 2^-16 of the row's largest get dq = 0 (they then add nothing to
any gradient whichever branch is taken; dcls_extra keeps its values there: its path has no ReLU).  At most 5 % of a case's rows, none at
B <= 3 - asserted on the reference, before anything runs on the device.

Tolerance.  Nobody had measured this chain against float64, so the bound is derived as for IPOT in tests/test_wpa_kernels_gpu.py: the same
chain in fp32 torch on the CPU (the accumulation onto the non-zero gradient arena included), e32 = its largest deviation from float64 per
output, allowed = 8 * max(e32, 2^-23 * max|ref|) - the factor covers another summation order in four chained GEMMs of K up to 1025 and
tanhf / rsqrtf against libm.  Measured deviation and allowance of every output of every case are collected in PARITY and written as JSON to
the file named by RMCL_HEADS_PARITY_OUT when that is set (profiles/heads_kernel_parity.json is such a dump).

Contract stated in include/rmcl.h and enforced on the host since this file exists: after a forward with RMCL_HEADS_NO_WGRAD the stash holds
no pooler input, so rmcl_heads_backward on that stash with grads32 != NULL returns -1 (test_backward_after_no_wgrad_forward_is_rejected)."""
import ctypes as C
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, stream  # noqa: E402

FACTOR = 8.0
CONFIGS = [(768, 128), (256, 64)]
BATCHES = [1, 3, 64, 256, 257, 1024, 1025]
NTOK = 8                                                                         # L = 4, cls, P = 3
HEAD_TENSORS = ("pool_w", "pool_b", "mh0_w", "mh0_b", "mh1_w", "mh1_b", "mh3_w")
SEED = 5                                                                         # chosen so that the ReLU-kink condition below holds in every case
NAN = float("nan")
PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_HEADS_PARITY_OUT")
    if out and PARITY:
        worst = max(((v[0] / v[1], f"{case}:{name}") for case, fig in PARITY.items() for name, v in fig.items() if v[1] > 0))
        with open(out, "w") as f:
            json.dump({"factor": FACTOR, "columns": ["kernel_dev", "allowed"], "largest_ratio": worst[0], "largest_ratio_at": worst[1],
                       "cases": PARITY}, f, indent=1, sort_keys=True)


def cpu_randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def make_dims(B, D, proj):
    return L.Dims(B=B, L=4, P=3, D=D, H=D // 64, layers=1, mlp=64, patch_k=3072, proj=proj, vocab=64, dtype=L.F32, exact=1, Pp=3)


# ------------------------------------------------------------------------------------------ inputs and references (CPU)
@functools.lru_cache(maxsize=None)
def arenas(D, proj):
    """Layout, tensor table {name: (offset, shape)}, two fp32 parameter arenas ("q": the query arena, which owns the pooler; "k": a second
    one for the MoCo head, so that head32 != pool32 runs too) and the start values of the gradient arena.  Weights ~ 0.03 randn and
    gamma = 1 + 0.1 randn: neither tanh nor the LayerNorm is saturated."""
    d, lay = make_dims(1, D, proj), L.Layout()
    lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    shapes = {"pool_w": (D, D), "pool_b": (D,), "mh0_w": (D, D), "mh0_b": (D,), "mh1_w": (D,), "mh1_b": (D,), "mh3_w": (proj, D)}
    table = {n: (getattr(lay, n), s) for n, s in shapes.items()}
    out = {}
    for i, name in enumerate(("q", "k")):
        a = cpu_randn(lay.total, seed=SEED + 10 * i + D, scale=0.03)
        a[lay.mh1_w:lay.mh1_w + D] = 1 + 0.1 * cpu_randn(D, seed=SEED + 10 * i + D + 1)
        out[name] = a
    return lay, table, out, cpu_randn(lay.total, seed=SEED + 50 + D, scale=0.01)


def weights(D, proj, head):
    """The seven tensors of one call: the pooler from the query arena, the projector from `head`."""
    _, table, par, _ = arenas(D, proj)
    return {n: par["q" if n.startswith("pool") else head][off:off + torch.Size(s).numel()].view(s) for n, (off, s) in table.items()}


def chain(x0, w, dtype, dq=None, dextra=None, G0=None):
    D = x0.shape[1]
    leaf = {n: t.to(dtype).clone().requires_grad_(True) for n, t in w.items()}
    x = x0.to(dtype).clone().requires_grad_(True)
    pooled = torch.tanh(x @ leaf["pool_w"].t() + leaf["pool_b"])
    h1 = pooled @ leaf["mh0_w"].t() + leaf["mh0_b"]
    pre = torch.nn.functional.layer_norm(h1, (D,), leaf["mh1_w"], leaf["mh1_b"], float(torch.tensor(1e-5, dtype=torch.float32)))
    z = torch.relu(pre) @ leaf["mh3_w"].t()
    q = z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    out = {"cls_feats": pooled.detach(), "q": q.detach(), "pre": pre.detach()}
    if dq is None and dextra is None:
        return out
    loss = 0
    if dq is not None:
        loss = loss + (q * dq.to(dtype)).sum()
    if dextra is not None:
        loss = loss + (pooled * dextra.to(dtype)).sum()
    loss.backward()
    out["dcls"] = x.grad
    for n in HEAD_TENSORS:                                                       # the arena ACCUMULATES: start value + gradient, in `dtype`
        out["G/" + n] = None if leaf[n].grad is None else G0[n].to(dtype) + leaf[n].grad
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(D, proj, B, head):
    """x0 = xn[:, 0], dq (zero in the rows marked for the ReLU kink), dcls_extra, the number of marked rows."""
    x0 = cpu_randn(B, D, seed=SEED + 1000 * B + D)
    pre = chain(x0, weights(D, proj, head), torch.float64)["pre"]
    marked = (pre.abs() < 2.0 ** -16 * pre.abs().amax(1, keepdim=True)).any(1)
    dq = cpu_randn(B, proj, seed=SEED + 1000 * B + D + 1)
    dq[marked] = 0
    return x0, dq, cpu_randn(B, D, seed=SEED + 1000 * B + D + 2), int(marked.sum())


@functools.lru_cache(maxsize=None)
def reference(D, proj, B, head, kind):
    """(float64 result, fp32 CPU twin) of one case; kind: "fwd", "dq", "extra" or "both"."""
    x0, dq, dextra, nmarked = case_inputs(D, proj, B, head)
    assert nmarked <= 0.05 * B and (B > 3 or nmarked == 0), (B, nmarked)
    _, table, _, g0 = arenas(D, proj)
    G0 = {n: g0[off:off + torch.Size(s).numel()].view(s) for n, (off, s) in table.items()}
    args = dict(dq=dq if kind in ("dq", "both") else None, dextra=dextra if kind in ("extra", "both") else None, G0=G0)
    w = weights(D, proj, head)
    return chain(x0, w, torch.float64, **args), chain(x0, w, torch.float32, **args)


def measure(fig, name, got, ref64, ref32):
    """Records [deviation, allowance] of one output and returns whether it is within the allowance."""
    got, ref64 = got.detach().double().cpu(), ref64.double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    if not torch.isfinite(got).all():
        fig[name] = [float("inf"), 0.0]
        return False
    e32 = float((ref32.double() - ref64).abs().max())
    allowed = FACTOR * max(e32, 2.0 ** -23 * float(ref64.abs().max()))
    dev = float((got - ref64).abs().max())
    fig[name] = [dev, allowed]
    return dev <= allowed


# ------------------------------------------------------------------------------------------ device side
@functools.lru_cache(maxsize=None)
def device_arenas(D, proj):
    _, _, par, g0 = arenas(D, proj)
    return {n: a.to(DEV) for n, a in par.items()}, g0.to(DEV)


class Call:
    """Buffers of one (D, proj, B) problem and the three entry points on them."""

    def __init__(self, D, proj, B, head):
        self.D, self.proj, self.B = D, proj, B
        self.d = make_dims(B, D, proj)
        par, self.g0 = device_arenas(D, proj)
        self.pool, self.head = par["q"], par[head]
        x0 = case_inputs(D, proj, B, head)[0]
        xn = torch.full((B, NTOK, D), 1e30)
        xn[:, 0] = x0
        self.xn = xn.to(DEV)
        self.stash_floats = int(lib.rmcl_heads_stash_bytes(C.byref(self.d))) // 4 + 1
        ws = int(lib.rmcl_workspace_bytes(C.byref(self.d)))
        # rmcl_heads_backward carves three [B, D] fp32 buffers from the start of the encoder workspace without a check of its own
        assert ws >= 3 * B * D * 4, (ws, B, D)
        self.work = torch.empty(ws // 4 + 1, device=DEV)
        self.new_stash()

    def new_stash(self):
        self.stash = torch.full((self.stash_floats,), NAN, device=DEV)

    def forward(self, flags=0, want_q=True, plain=False):
        cls, q = torch.full((self.B, self.D), NAN, device=DEV), torch.full((self.B, self.proj), NAN, device=DEV)
        a = (C.byref(self.d), P(self.pool), P(self.head), P(self.xn), P(self.stash), P(cls), P(q if want_q else None))
        if plain:
            check(lib.rmcl_heads_forward(*a, stream()), "heads_forward")
        else:
            check(lib.rmcl_heads_forward2(*a, flags, stream()), "heads_forward2")
        return cls, q

    def backward(self, dq, dextra, G):
        self.work[:3 * self.B * self.D] = NAN
        dcls = torch.full((self.B, self.D), NAN, device=DEV)
        rc = lib.rmcl_heads_backward(C.byref(self.d), P(self.pool), P(self.head), P(self.stash), P(dq), P(dextra), P(dcls), P(G),
                                     P(self.work), stream())
        return rc, dcls


class skinny_form:
    """rmcl_tune_set key 6 around a region (process-global: restored on the way out)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        check(lib.rmcl_tune_set(6, self.form), "tune_set")

    def __exit__(self, *exc):
        check(lib.rmcl_tune_set(6, -1), "tune_set")


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("form", [-1, 0])
@pytest.mark.parametrize("flags", [0, L.HEADS_NO_WGRAD])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Dp", CONFIGS, ids=["D768", "D256"])
def test_heads_forward_against_fp64(Dp, B, flags, form):
    D, proj = Dp
    bad = {}
    with skinny_form(form):
        for head in ("q", "k"):
            ref64, ref32 = reference(D, proj, B, head, "fwd")
            c = Call(D, proj, B, head)
            cls, q = c.forward(flags)
            fig = PARITY.setdefault(f"fwd/D{D}/B{B}/flags{flags}/form{form}/head_{head}", {})
            ok = measure(fig, "cls_feats", cls, ref64["cls_feats"], ref32["cls_feats"])
            ok &= measure(fig, "q", q, ref64["q"], ref32["q"])
            print(fig)
            if not ok:
                bad[head] = fig
            # q = NULL stops after the pooler: the same cls_feats, the q buffer untouched
            c.new_stash()
            cls2, q2 = c.forward(flags, want_q=False)
            assert torch.equal(bits(cls2), bits(cls)) and torch.isnan(q2).all()
            # rmcl_heads_forward is rmcl_heads_forward2(..., 0); the strided in-place read of NO_WGRAD is the same GEMM on the same values
            c.new_stash()
            cls3, q3 = c.forward(0, plain=(flags == 0))
            assert torch.equal(bits(cls3), bits(cls)) and torch.equal(bits(q3), bits(q))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ backward
KIND = {"dq": "dq", "extra": "extra", "both": "both", "both_nog": "both"}


@pytest.mark.parametrize("form", [-1, 0])
@pytest.mark.parametrize("case", ["dq", "extra", "both", "both_nog"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Dp", CONFIGS, ids=["D768", "D256"])
def test_heads_backward_against_fp64(Dp, B, case, form):
    """dq only / dcls_extra only (dq = NULL: through tanh only) / both (added through the row scatter) / both without a gradient arena.
    The two "both" cases take the projector from the second arena (head32 != pool32).  With an arena: it starts as random values, the
    seven head tensors must move by the float64 gradient and every other element must keep its bits."""
    D, proj = Dp
    kind, head = KIND[case], "k" if case.startswith("both") else "q"
    ref64, ref32 = reference(D, proj, B, head, kind)
    _, dq, dextra, _ = case_inputs(D, proj, B, head)
    dq = dq.to(DEV) if kind in ("dq", "both") else None
    dextra = dextra.to(DEV) if kind in ("extra", "both") else None
    _, table, _, _ = arenas(D, proj)
    fig = PARITY.setdefault(f"bwd/D{D}/B{B}/{case}/form{form}", {})
    ok = True
    with skinny_form(form):
        c = Call(D, proj, B, head)
        c.forward(0)
        G = None if case == "both_nog" else c.g0.clone()
        rc, dcls = c.backward(dq, dextra, G)
        check(rc, "heads_backward")
        ok &= measure(fig, "dcls", dcls, ref64["dcls"], ref32["dcls"])
        if G is not None:
            others = bits(G) != bits(c.g0)
            for n, (off, s) in table.items():
                cnt = torch.Size(s).numel()
                others[off:off + cnt] = False
                if ref64["G/" + n] is None:                                      # no gradient reaches it (dq = NULL): not one bit moves
                    assert torch.equal(bits(G[off:off + cnt]), bits(c.g0[off:off + cnt])), n
                else:
                    ok &= measure(fig, n, G[off:off + cnt].view(s), ref64["G/" + n], ref32["G/" + n])
            assert not bool(others.any()), "an element outside the seven head tensors changed"
        else:
            # the pass that keeps no pooler input (NO_WGRAD forward) is legal exactly here and gives the same dcls
            c.new_stash()
            c.forward(L.HEADS_NO_WGRAD)
            rc, dcls2 = c.backward(dq, dextra, None)
            check(rc, "heads_backward after NO_WGRAD")
            ok &= measure(fig, "dcls_no_wgrad", dcls2, ref64["dcls"], ref32["dcls"])
            assert torch.equal(bits(dcls2), bits(dcls))
    print(fig)
    assert ok, fig


def test_backward_needs_dq_or_dcls_extra():
    c = Call(256, 64, 3, "q")
    c.forward(0)
    rc, dcls = c.backward(None, None, None)
    assert rc == -1 and b"neither dq nor dcls_extra" in lib.rmcl_last_error()
    assert torch.isnan(dcls).all()


def test_backward_after_no_wgrad_forward_is_rejected():
    """The header's contract (a RMCL_HEADS_NO_WGRAD forward is followed by a backward with grads32 = NULL) is checked on the host, from
    a record of which stash buffers last saw such a forward: no device read, no synchronise.  A later plain forward on the same stash
    makes the weight-gradient backward legal again."""
    D, proj, B = 256, 64, 3
    c = Call(D, proj, B, "q")
    _, dq, dextra, _ = case_inputs(D, proj, B, "q")
    dq, dextra = dq.to(DEV), dextra.to(DEV)
    c.forward(L.HEADS_NO_WGRAD)
    G = c.g0.clone()
    rc, dcls = c.backward(dq, dextra, G)
    assert rc == -1 and b"NO_WGRAD" in lib.rmcl_last_error()
    assert torch.isnan(dcls).all() and torch.equal(bits(G), bits(c.g0))
    rc, _ = c.backward(dq, dextra, None)
    check(rc, "heads_backward, no arena")
    c.forward(0)
    rc, dcls = c.backward(dq, dextra, G)
    check(rc, "heads_backward after a plain forward")
    ref64, ref32 = reference(D, proj, B, "q", "both")
    assert measure({}, "dcls", dcls, ref64["dcls"], ref32["dcls"])
