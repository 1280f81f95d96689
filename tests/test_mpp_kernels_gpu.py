"""-m gpu: the masked-patch-prediction kernels (csrc/mpp.hip: rmcl_mpp_ws_floats, rmcl_mpp_labels, rmcl_mpp_compact, rmcl_mpp_forward,
rmcl_mpp_backward, rmcl_mpp_logits) against torch in fp64, and the mask-token substitution passes (rmcl_encoder_forward_mpp,
rmcl_encoder_backward_mpp, rmcl_visual_embed_mpp) against the CPU oracle (tests/mpp_oracle.py)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P, I64  # noqa: E402
from rmcl_amd.runtime import mpp_layout, stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_mlm_itm_mpp, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from tests import mpp_oracle as M  # noqa: E402

DEV = "cuda:0"
C = ctypes
F = C.c_float


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ---- labels -------------------------------------------------------------------------------------------------------------------------
def _labels(img, sel=None, counts=None, Pn=None):
    B, _, H, W = img.shape
    G = (H // 32) * (W // 32)
    Pn = G if Pn is None else Pn
    out = torch.full((B, Pn, 3), -7, dtype=torch.int32, device=DEV)
    d = img.to(DEV).contiguous()
    if sel is None:
        check(lib.rmcl_mpp_labels(P(d), B, H, W, None, None, 0, W // 32, Pn, P(out), stream_ptr()))
    else:
        s, c = sel.to(DEV, torch.int32).contiguous(), counts.to(DEV, torch.int32).contiguous()
        check(lib.rmcl_mpp_labels(P(d), B, H, W, P(s), P(c), s.shape[1], W // 32, Pn, P(out), stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().long()


def _exact_image(shape, seed):
    """pixels that are multiples of 1 / 64 in [-1, 1]: every summation order gives the same fp32 patch mean"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, shape, generator=g).float() / 64.0


def test_labels_exact_dense():
    img = _exact_image((2, 3, 64, 64), 1)
    img[0, :, :32, :32] = 1.0                                           # an all-ones patch: 255
    img[1, :, 32:, 32:] = -1.0                                          # an all-minus-ones patch: 0
    got = _labels(img)
    want = M.patch_labels(img)
    assert torch.equal(want, M.patch_means_fp64(img).floor().long())    # (the reference formula is exact on such data)
    assert torch.equal(got, want)
    assert got[0, 0].tolist() == [255, 255, 255] and got[1, 3].tolist() == [0, 0, 0]


def test_labels_exact_ragged_selection():
    sizes = [(96, 128), (64, 64), (32, 96)]
    img = _exact_image((3, 3, 96, 128), 2)
    for b, (h, w) in enumerate(sizes):
        img[b, :, h:, :] = 0
        img[b, :, :, w:] = 0
    img[1, :, :32, :32] = 1.0
    img[2, :, :32, 32:64] = -1.0
    cfg = O.default_config(max_image_len=-1)
    sel, valid = M.selection(img, cfg)
    counts = valid.sum(1)
    assert counts.tolist() == [12, 4, 3] and sel.shape[1] == 12
    got = _labels(img, sel, counts, Pn=12)
    full = M.patch_labels(img)
    want = torch.gather(full, 1, sel.unsqueeze(-1).expand(-1, -1, 3)).clone()
    want[~valid] = -100
    assert torch.equal(got, want)
    assert got[1, 0].tolist() == [255] * 3 and got[2, 1].tolist() == [0] * 3 and bool((got[2, 3:] == -100).all())


def test_labels_generic_float_pixels():
    g = torch.Generator().manual_seed(3)
    img = torch.rand(4, 3, 96, 96, generator=g) * 2 - 1
    v = M.patch_means_fp64(img)
    band = (v - v.round()).abs() < 1e-3
    ref32 = M.patch_labels(img)
    assert torch.equal(ref32[~band], v.floor().long()[~band])            # the reference's fp32 formula agrees with fp64 outside the band
    assert float(band.float().mean()) <= 0.01
    got = _labels(img)
    assert torch.equal(got[~band], v.floor().long()[~band])
    assert bool(((got - v.floor().long()).abs() <= 1)[band].all())


# ---- compaction ---------------------------------------------------------------------------------------------------------------------
def _compact(labels, masked, Lt, N, all_rows=0):
    B, Pn, _ = labels.shape
    cap = (B * (Pn + 1) + 127) // 128 * 128
    idx = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    lab = torch.full((cap, 3), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    lb, mk = labels.to(DEV, torch.int32).contiguous(), masked.to(DEV, torch.int32).contiguous()
    check(lib.rmcl_mpp_compact(P(lb), P(mk), B, Pn, Lt, N, all_rows, cap, P(idx), P(lab), P(cnt), stream_ptr()))
    torch.cuda.synchronize()
    return idx.cpu().long(), lab.cpu().long(), cnt.cpu().tolist()


def _ragged_case(seed=4, Pn=12, B=4):
    """labels with pad slots and the mask cases: sample 0 nothing masked, sample 1 first and last valid slot, sample 2 a masked pad slot and
    one valid slot, sample 3 random"""
    g = torch.Generator().manual_seed(seed)
    counts = [Pn, 7, 5, Pn]
    labels = torch.randint(0, 256, (B, Pn, 3), generator=g)
    masked = torch.rand(B, Pn, generator=g) < 0.3
    for b, c in enumerate(counts):
        labels[b, c:] = -100
    masked[0] = False
    masked[1] = False
    masked[1, 0] = masked[1, 6] = True
    masked[2] = False
    masked[2, 2] = masked[2, 9] = True                                   # slot 9 is a pad slot
    masked[3, 1] = True
    return labels, masked, counts


def _compact_ref(labels, masked, Lt, N):
    on = masked & (labels != -100).any(-1)
    b, j = on.nonzero(as_tuple=True)
    return b * N + Lt + 1 + j, labels[on]


def test_compaction_ragged_masks_and_empty():
    labels, masked, counts = _ragged_case()
    Lt, N = 5, 5 + 1 + 12
    idx, lab, cnt = _compact(labels, masked, Lt, N)
    ri, rl = _compact_ref(labels, masked, Lt, N)
    n = ri.numel()
    assert cnt == [n, 0] and torch.equal(idx[:n], ri) and torch.equal(lab[:n], rl)
    assert bool((idx[n:] == -1).all()) and bool((lab[n:] == -100).all())
    assert (1 * N + Lt + 1) in idx.tolist() and (1 * N + Lt + 7) in idx.tolist() and (2 * N + Lt + 10) not in idx.tolist()
    assert not any(0 <= int(i) < N for i in idx[:n])                      # sample 0: nothing
    idx0, lab0, cnt0 = _compact(labels, torch.zeros_like(masked), Lt, N)
    assert cnt0 == [0, 0] and bool((idx0 == -1).all()) and bool((lab0 == -100).all())
    # the dense-logits listing: every image row, the cls row first; labels only where the compacted form has them
    idxa, laba, cnta = _compact(labels, masked, Lt, N, all_rows=1)
    assert cnta[0] == 4 * 13
    want = torch.stack([torch.arange(13) + b * N + Lt for b in range(4)]).flatten()
    assert torch.equal(idxa[:52], want)
    la = torch.full((4, 13, 3), -100)
    la[:, 1:][masked & (labels != -100).any(-1)] = rl
    assert torch.equal(laba[:52], la.reshape(52, 3))


def test_compaction_counts_and_skips_labels_out_of_range():
    labels, masked, counts = _ragged_case()
    labels[3, 1, 2] = 256
    labels[1, 0, 0] = -1
    Lt, N = 5, 18
    idx, lab, cnt = _compact(labels, masked, Lt, N)
    ok = labels.clone()
    m2 = masked.clone()
    m2[3, 1] = m2[1, 0] = False
    ri, rl = _compact_ref(ok, m2, Lt, N)
    assert cnt == [ri.numel(), 2] and torch.equal(idx[:ri.numel()], ri) and torch.equal(lab[:ri.numel()], rl)


# ---- head ---------------------------------------------------------------------------------------------------------------------------
def _head_case(n, D, seed, tie=False):
    """n masked slots among B x 16 image slots of an xn with 24 token rows per sample (7 text rows); a head with peaked logits"""
    Lt, Pn = 7, 16
    N = Lt + 1 + Pn
    B = max(2, -(-n // Pn))
    h, specs, total = mpp_layout({"hidden_size": D}, 0)
    g = torch.Generator().manual_seed(seed)
    arena = torch.zeros(total)
    w = {}
    for name, off, shape in specs:
        if name.endswith("LayerNorm.weight"):
            t = 1 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("decoder.weight"):
            t = 4.0 * torch.randn(shape, generator=g) / D ** 0.5
        elif len(shape) == 2:
            t = torch.randn(shape, generator=g) / D ** 0.5
        else:
            t = 0.3 * torch.randn(shape, generator=g)
        if tie and name.endswith("decoder.weight"):
            t[256 + 250] = t[256 + 5]                              # two identical columns of channel 1, in different lanes
        if tie and name.endswith("decoder.bias"):
            t[256 + 5] = t[256 + 250] = 30.0                       # ... that win every row: the FIRST maximum is class 5
        arena[off:off + t.numel()] = t.flatten()
        w[name] = t
    xn = torch.randn(B * N, D, generator=g)
    labels = torch.randint(0, 256, (B, Pn, 3), generator=g)
    masked = torch.zeros(B * Pn, dtype=torch.bool)
    masked[torch.randperm(B * Pn, generator=g)[:n]] = True
    return h, specs, arena, w, xn, labels, masked.view(B, Pn), Lt, N


def _run_head(h, arena, xn, labels, masked, Lt, N, dtype, gscale=1.0):
    B, Pn, _ = labels.shape
    n = int(masked.sum())
    rows = max(128, (n + 127) // 128 * 128)
    cap = (B * (Pn + 1) + 127) // 128 * 128
    rows = min(rows, cap)
    dt = L.BF16 if dtype == "bf16" else L.F32
    a = arena.to(DEV)
    lp = a.to(torch.bfloat16) if dt == L.BF16 else None
    i32 = lambda *k: torch.full(k, -7, dtype=torch.int32, device=DEV)
    f32 = lambda *k: torch.full(k, float("nan"), dtype=torch.float32, device=DEV)
    idx, lab, cnt = i32(cap), i32(cap, 3), i32(2)
    lse, rl, am, stats = f32(rows, 3), f32(rows), i32(rows, 3), f32(3)
    ws = torch.empty(int(lib.rmcl_mpp_ws_floats(C.byref(h), rows)), device=DEV)
    G = torch.zeros_like(a)
    dxn = torch.zeros(xn.shape, device=DEV)
    x = xn.to(DEV)
    lb, mk = labels.to(DEV, torch.int32).contiguous(), masked.to(DEV, torch.int32).contiguous()
    gs = torch.tensor([gscale], device=DEV)
    check(lib.rmcl_mpp_compact(P(lb), P(mk), B, Pn, Lt, N, 0, cap, P(idx), P(lab), P(cnt), stream_ptr()))
    check(lib.rmcl_mpp_forward(C.byref(h), P(a), P(lp), dt, P(x), P(idx), P(lab), P(cnt), rows, P(ws), P(lse), P(rl), P(am), P(stats), stream_ptr()))
    check(lib.rmcl_mpp_backward(C.byref(h), P(a), P(lp), dt, P(idx), P(lab), P(cnt), rows, P(ws), P(lse), F(1.0), P(gs), P(G), P(dxn), stream_ptr()))
    logits = torch.empty(max(n, 1), 768, device=DEV)
    check(lib.rmcl_mpp_logits(C.byref(h), P(ws), rows, max(n, 1), P(logits), stream_ptr()))
    torch.cuda.synchronize()
    return dict(idx=idx, lab=lab, cnt=cnt, lse=lse, rowloss=rl, argmax=am, stats=stats, G=G, dxn=dxn, logits=logits, n=n, rows=rows)


def _fp64_head(w, xn, labels, masked, Lt, N, dtype, gscale):
    """The head in fp64 with autograd; bf16 engine: the decoder's operands are what the kernels multiply (the bf16 shadow of decoder.weight
    and h rounded to bf16, straight-through for the gradient), as _fp64_reference of tests/test_mlm_gpu.py does."""
    wd = {k: v.double().requires_grad_(True) for k, v in w.items()}
    x0 = xn.double().requires_grad_(True)
    rows_i, lab = _compact_ref(labels, masked, Lt, N)
    n = rows_i.numel()
    hh = M.mpp_transform(wd, x0[rows_i])
    Wd = wd["mpp_score.decoder.weight"]
    if dtype == "bf16":
        hh = hh + (bf16_round(hh.detach().float()).double() - hh.detach())
        Wd = Wd + (bf16_round(Wd.detach().float()).double() - Wd.detach())
    z = hh @ Wd.t() + wd["mpp_score.decoder.bias"]
    ce = torch.nn.functional.cross_entropy(z.reshape(-1, 256), lab.reshape(-1), reduction="none").reshape(n, 3)
    (gscale * ce.sum() / (3 * n)).backward()
    return dict(z=z.detach(), ce=ce.detach(), lse=torch.logsumexp(z.detach().reshape(n, 3, 256), 2), w=wd, x0=x0, rows_i=rows_i, lab=lab, n=n)


# the bounds of tests/test_mlm_gpu.py for the same quantities and dtypes (same arithmetic class: fp32 products over K = D against fp64;
# bf16: the same bf16 operands on both sides, dz rounded to bf16 before the dW / dh products and the dbias sums)
KTOL = {"f32": dict(z=1e-4, loss=1e-5, grad=2e-4), "bf16": dict(z=5e-3, loss=2e-3, grad=2e-2)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_mpp_head_matches_torch_fp64(n, D, dtype):
    h, specs, arena, w, xn, labels, masked, Lt, N = _head_case(n, D, 2000 + n + D)
    r = _run_head(h, arena, xn, labels, masked, Lt, N, dtype, gscale=0.5)
    ref = _fp64_head(w, xn, labels, masked, Lt, N, dtype, 0.5)
    tol = KTOL[dtype]
    assert r["cnt"].tolist() == [n, 0] and ref["n"] == n
    assert torch.equal(r["idx"][:n].cpu().long(), ref["rows_i"]) and torch.equal(r["lab"][:n].cpu().long(), ref["lab"])
    zmax = max(1.0, float(ref["z"].abs().max()))
    z = r["logits"][:n].cpu().double()
    ez = float((z - ref["z"]).abs().max())
    el = float((r["lse"][:n].cpu().double() - ref["lse"]).abs().max())
    er = float((r["rowloss"][:n].cpu().double() - ref["ce"].sum(1)).abs().max())
    print(f"mpp head n={n} D={D} {dtype}: |dz|max {ez:.3e} lse {el:.3e} rowloss {er:.3e} (|z|max {zmax:.2f})")
    assert ez < tol["z"] * zmax and el < tol["z"] * zmax and er < 3 * 2 * tol["z"] * zmax
    assert bool((r["rowloss"][n:] == 0).all()) and bool((r["argmax"][n:] == -1).all()) and bool((r["lse"][n:] == 0).all())
    # argmax: the reference's wherever its top-two gap is clear of the logits tolerance; and the first maximum of the kernels' own logits
    zg = ref["z"].reshape(n, 3, 256)
    top2 = zg.topk(2, dim=2)
    clear = (top2.values[..., 0] - top2.values[..., 1]) > 2 * tol["z"] * zmax
    am = r["argmax"][:n].cpu().long()
    assert bool(((am >= 0) & (am < 256)).all())
    assert torch.equal(am[clear], top2.indices[..., 0][clear])
    assert torch.equal(am, r["logits"][:n].reshape(n, 3, 256).argmax(dim=2).cpu())
    st = r["stats"].cpu().double()
    assert abs(float(st[0]) - float(ref["ce"].mean())) < tol["loss"] * float(ref["ce"].mean())
    assert float(st[1]) == float((am == ref["lab"]).sum()) and float(st[2]) == 3 * n
    for name, off, shape in specs:
        if name == "transformer.mask_token":
            assert torch.count_nonzero(r["G"][off:off + D]) == 0         # the head never touches the mask token's gradient
            continue
        got = r["G"][off:off + w[name].numel()].view(shape).cpu().double()
        want = ref["w"][name].grad
        err = float((got - want).abs().max())
        print(f"   grad {name}: {err:.3e} of {float(want.abs().max()):.3e}")
        assert err < tol["grad"] * float(want.abs().max()) + 1e-12, name
    gx = ref["x0"].grad
    assert float((r["dxn"].cpu().double() - gx).abs().max()) < tol["grad"] * float(gx.abs().max())
    other = torch.ones(xn.shape[0], dtype=torch.bool)
    other[ref["rows_i"]] = False
    assert torch.count_nonzero(r["dxn"].cpu()[other]) == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [256, 768])
def test_mpp_head_all_ignored_batch(D, dtype):
    """n = 0: NaN loss like F.cross_entropy over an all-ignored batch, nothing but zeros added to the gradient arena, no NaN in dxn"""
    h, specs, arena, w, xn, labels, masked, Lt, N = _head_case(0, D, 7)
    r = _run_head(h, arena, xn, labels, masked, Lt, N, dtype)
    assert r["cnt"].tolist() == [0, 0] and bool(torch.isnan(r["stats"][0])) and float(r["stats"][2]) == 0
    assert torch.count_nonzero(r["G"]) == 0 and torch.count_nonzero(r["dxn"]) == 0
    assert bool(torch.isfinite(r["G"]).all()) and bool(torch.isfinite(r["dxn"]).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mpp_argmax_ties_go_to_the_first_class(dtype):
    h, specs, arena, w, xn, labels, masked, Lt, N = _head_case(37, 768, 5, tie=True)
    r = _run_head(h, arena, xn, labels, masked, Lt, N, dtype)
    lg = r["logits"][:37]
    assert torch.equal(lg[:, 256 + 5], lg[:, 256 + 250])                  # identical operands: identical bits in both columns
    assert bool((r["argmax"][:37, 1] == 5).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mpp_head_is_bit_reproducible(dtype):
    h, specs, arena, w, xn, labels, masked, Lt, N = _head_case(300, 768, 9)
    a = _run_head(h, arena, xn, labels, masked, Lt, N, dtype)
    b = _run_head(h, arena, xn, labels, masked, Lt, N, dtype)
    for k in ("idx", "lab", "cnt", "lse", "rowloss", "argmax", "stats", "G", "dxn", "logits"):
        assert torch.equal(a[k], b[k]), k


def test_labels_are_bit_reproducible():
    g = torch.Generator().manual_seed(12)
    img = torch.rand(4, 3, 96, 96, generator=g) * 2 - 1
    assert torch.equal(_labels(img), _labels(img))


def test_null_operands_are_rejected_before_any_launch():
    h, _, _ = mpp_layout({"hidden_size": 768}, 0)
    buf = (C.c_float * 16)()
    ib = (C.c_int32 * 16)()
    hp = C.byref(h)

    def rejected(rc, what):
        msg = lib.rmcl_last_error()
        assert rc == -1 and msg and what.encode() in msg, (what, rc, msg)

    rejected(lib.rmcl_mpp_labels(None, 1, 32, 32, None, None, 0, 1, 1, ib, None), "mpp_labels")
    rejected(lib.rmcl_mpp_labels(buf, 1, 32, 32, ib, None, 1, 1, 1, ib, None), "mpp_labels")
    rejected(lib.rmcl_mpp_labels(buf, 1, 32, 48, None, None, 0, 1, 1, ib, None), "mpp_labels")
    rejected(lib.rmcl_mpp_compact(ib, None, 1, 1, 1, 3, 0, 128, ib, ib, ib, None), "mpp_compact")
    rejected(lib.rmcl_mpp_forward(hp, buf, None, L.F32, None, ib, ib, ib, 128, buf, buf, buf, ib, buf, None), "mpp_forward")
    rejected(lib.rmcl_mpp_forward(hp, buf, None, L.BF16, buf, ib, ib, ib, 128, buf, buf, buf, ib, buf, None), "mpp_forward")
    rejected(lib.rmcl_mpp_forward(hp, buf, None, L.F32, buf, ib, ib, ib, 100, buf, buf, buf, ib, buf, None), "mpp_forward")
    rejected(lib.rmcl_mpp_backward(hp, buf, None, L.F32, ib, ib, ib, 128, None, buf, F(1.0), None, None, None, None), "mpp_backward")
    rejected(lib.rmcl_mpp_logits(hp, None, 128, 1, buf, None), "mpp_logits")
    d = L.Dims(B=1, L=4, P=3, D=64, H=1, layers=1, mlp=64, patch_k=64, proj=64, vocab=64, dtype=L.F32, exact=1, Pp=3)
    dp = C.byref(d)
    rejected(lib.rmcl_encoder_forward_mpp(dp, L.MODE_INFER, None, None, buf, buf, buf, ib, None, buf, buf, C.c_uint32(0), F(0.0), None, None,
                                          ib, I64(0), None), "encoder_forward")
    rejected(lib.rmcl_encoder_forward_mpp(dp, L.MODE_INFER | L.MODE_CLS_TAIL, buf, None, buf, buf, buf, ib, None, buf, buf, C.c_uint32(0), F(0.0),
                                          None, None, ib, I64(0), None), "encoder_forward_mpp")
    rejected(lib.rmcl_encoder_backward_mpp(dp, L.MODE_DATA, buf, None, buf, buf, ib, None, buf, buf, None, None, None, C.c_uint32(0), F(0.0),
                                           None, None, ib, I64(0), None), "encoder_backward")
    rejected(lib.rmcl_visual_embed_mpp(dp, None, None, buf, None, buf, buf, ib, ib, I64(0), None), "visual_embed")


# ---- the substitution pass against the CPU oracle -------------------------------------------------------------------------------------
def _module(ocfg, p, dtype, drop_rate=0.0, **over):
    kw = dict(num_layers=ocfg["num_layers"], per_gpu_batchsize=ocfg["per_gpu_batchsize"], drop_rate=drop_rate, max_steps=100, warmup_steps=0,
              image_size=ocfg["image_size"], max_image_len=ocfg.get("max_image_len", -1), loss_names=_loss_names({"mpp": 1}))
    kw.update(over)
    m = ViLTransformerSS(task_mlm_itm_mpp(**kw), device=DEV, compute_dtype=dtype)
    sd = {n: t.to(DEV) for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    m.train()
    return m


def _pass_case(kind):
    if kind == "dense":
        ocfg = O.default_config(num_layers=2, per_gpu_batchsize=4, image_size=64, max_image_len=-1)
        batch = O.synthetic_batch(ocfg, 4, 21, ragged_text=True)
    else:
        ocfg = O.default_config(num_layers=2, per_gpu_batchsize=4, max_image_len=-1)
        batch = O.synthetic_batch(ocfg, 4, 22, ragged_text=True, sizes=[(96, 128), (64, 64), (32, 96), (96, 96)])
    p = dict(O.init_params(ocfg, 23), **M.mpp_init_params(ocfg, 24))
    return ocfg, p, batch


PASS_GRADS = ("transformer.mask_token", "transformer.patch_embed.proj.weight", "transformer.patch_embed.proj.bias", "transformer.pos_embed",
              "transformer.cls_token")
PTOL = {"f32": dict(x=2e-3, grad=5e-3), "bf16": dict(x=0.1, grad=0.2)}       # (the encoder-pass bounds of tests/test_path_gpu.py)


def _run_pass(m, batch, masked, replaced, pdrop):
    """one FULL-mode pass with the substitution and a fixed xn-gradient on the image rows; returns (xn, grads, dropout masks)"""
    eng = m.engine
    eng.dropout_on = pdrop > 0
    img = batch["image"][0].to(DEV)
    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], img, tag="mpp")
    mp = eng.mpp_bind(eng.mpp_bufs(pb.B, "mpp", pb.d.P), img.float().contiguous(), pb, masked, replaced)
    op = eng.make_operand(pb, out=pb.patchesT_full)
    eng.zero_grads()
    eng.encoder_forward(pb, key=False, mode=L.MODE_FULL, patchesT=op, replaced=mp.replaced)
    d = pb.d
    N = d.L + 1 + d.P
    g = torch.Generator().manual_seed(31)
    dxn = torch.zeros(pb.B, N, d.D)
    dxn[:, d.L:] = torch.randn(pb.B, d.P + 1, d.D, generator=g) * pb.co_mask[:, d.L:].cpu().unsqueeze(-1)
    dpat = torch.empty_like(pb.patchesT_full)
    eng.encoder_backward(pb, L.MODE_FULL, op, dxn.to(DEV).view(pb.B * N, d.D).contiguous(), cls_only=False, dpatches=dpat, replaced=mp.replaced)
    torch.cuda.synchronize()
    seed, pp = pb.drop[L.MODE_FULL]
    drop = None
    if pdrop > 0:
        def mask(shape, layer, site):
            x = torch.ones(shape, device=DEV)
            check(lib.rmcl_dropout_mask_apply(P(x), I64(x.numel()), C.c_uint32(seed), layer, site, F(pdrop), stream_ptr()))
            return x.cpu()
        drop = {"text": mask((pb.B, d.L, d.D), 0, 3), "image": mask((pb.B, d.P + 1, d.D), 0, 4)}
        for l in range(2):
            drop[l] = {"proj": mask((pb.B, N, d.D), l, 0), "hidden": mask((pb.B, N, 4 * d.D), l, 1), "fc2": mask((pb.B, N, d.D), l, 2)}
    grads = {n_: prm.grad.clone().cpu() for n_, prm in m.named_parameters() if n_ in PASS_GRADS}
    return pb.xn.view(pb.B, N, d.D).cpu().clone(), grads, drop, dxn, mp, dpat.float().cpu(), pb


@pytest.mark.parametrize("pdrop", [0.0, 0.1])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["dense", "ragged"])
def test_substitution_pass_matches_oracle(kind, dtype, pdrop):
    ocfg, p, batch = _pass_case(kind)
    img = batch["image"][0]
    masked, replaced = M.make_masks(img, ocfg, 25, "ragged")
    m = _module(ocfg, p, dtype, drop_rate=pdrop)
    xn, grads, drop, dxn, mp, dpat, pb = _run_pass(m, batch, masked, replaced, pdrop)
    sel, valid = M.selection(img, ocfg)
    assert torch.equal(mp.replaced.cpu().bool(), torch.gather(replaced, 1, sel) & valid)      # gathered through the selection, pads 0
    pp = {n_: (t.clone().requires_grad_(True) if n_ in PASS_GRADS else t) for n_, t in p.items()}
    out = M.infer_masked(pp, ocfg, batch["text_ids"], batch["text_masks"], img, replaced, drop=drop)
    Lt = batch["text_ids"].shape[1]
    tol = PTOL[dtype]
    im = out["image_masks"].bool()
    ex = float((xn[:, Lt:][im] - out["image_feats"].detach()[im]).abs().max())
    print(f"substitution {kind} {dtype} p={pdrop}: xn image rows {ex:.3e} of {float(out['image_feats'].abs().max()):.2f}")
    assert ex < tol["x"] * max(1.0, float(out["image_feats"].abs().max()))
    (out["image_feats"] * dxn[:, Lt:]).sum().backward()
    for n_ in PASS_GRADS:
        want = pp[n_].grad
        err = float((grads[n_] - want).abs().max())
        print(f"   grad {n_}: {err:.3e} of {float(want.abs().max()):.3e}")
        assert err <= tol["grad"] * float(want.abs().max()) + 1e-8, n_
    assert float(grads["transformer.mask_token"].abs().max()) > 0
    # a replaced patch receives no pixel gradient
    rows = mp.replaced.cpu().bool().flatten()
    assert torch.count_nonzero(dpat[rows]) == 0 and torch.count_nonzero(dpat[~rows]) > 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_replaced_none_is_the_plain_pass_and_replaced_all_stops_the_patch_gradient(dtype):
    ocfg, p, batch = _pass_case("ragged")
    img = batch["image"][0]
    m = _module(ocfg, p, dtype)
    eng = m.engine
    G = (img.shape[2] // 32) * (img.shape[3] // 32)
    none = torch.zeros(4, G, dtype=torch.bool)
    xn0, g0, _, dxn, mp, dpat0, pb = _run_pass(m, batch, none, none, 0.0)
    # the plain entry points on the same buffers: identical bits, forward and backward
    op = eng.make_operand(pb, out=pb.patchesT_full)
    eng.zero_grads()
    eng.encoder_forward(pb, key=False, mode=L.MODE_FULL, patchesT=op)
    assert torch.equal(pb.xn.cpu().view_as(xn0), xn0)
    N = pb.d.L + 1 + pb.d.P
    eng.encoder_backward(pb, L.MODE_FULL, op, dxn.to(DEV).view(pb.B * N, pb.d.D).contiguous(), cls_only=False, dpatches=None)
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    for n_ in PASS_GRADS[1:]:                                            # (the embedding gradients meet in float atomics: equal up to their order)
        a, b = params[n_].grad.cpu(), g0[n_]
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), n_
    assert torch.count_nonzero(g0["transformer.mask_token"]) == 0
    every = torch.ones(4, G, dtype=torch.bool)
    xn1, g1, _, _, mp1, dpat1, _ = _run_pass(m, batch, every, every, 0.0)
    assert torch.count_nonzero(g1["transformer.patch_embed.proj.weight"]) == 0           # exactly zero
    assert torch.count_nonzero(g1["transformer.patch_embed.proj.bias"]) == 0 and torch.count_nonzero(dpat1) == 0
    assert float(g1["transformer.mask_token"].abs().max()) > 0 and float(g1["transformer.pos_embed"].abs().max()) > 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mask_token_gradient_and_patch_rows_are_bit_reproducible(dtype):
    """two identical passes with dropout: the same bits in xn, in the mask token's gradient (per-sample partials merged in sample order,
    no atomics) and in the pixel gradient with its zeroed replaced rows"""
    ocfg, p, batch = _pass_case("ragged")
    masked, replaced = M.make_masks(batch["image"][0], ocfg, 25, "ragged")
    m = _module(ocfg, p, dtype, drop_rate=0.1)
    m.engine.pass_counter = 100
    xa, ga, _, _, _, da, _ = _run_pass(m, batch, masked, replaced, 0.1)
    m.engine.pass_counter = 100                                          # the same dropout seed
    xb, gb, _, _, _, db, _ = _run_pass(m, batch, masked, replaced, 0.1)
    assert torch.equal(xa, xb) and torch.equal(da, db)
    assert torch.equal(ga["transformer.mask_token"], gb["transformer.mask_token"]) and float(ga["transformer.mask_token"].abs().max()) > 0


def test_substitution_pass_with_streaming_attention_above_256_tokens():
    """N = 257: 40 text tokens + 1 + 216 patches (a 384 x 576 image) on a long_sequences bf16 engine (RMCL_MODE_STREAM_ATTN)"""
    ocfg = O.default_config(num_layers=2, per_gpu_batchsize=2, max_image_len=-1)
    g = torch.Generator().manual_seed(41)
    batch = O.synthetic_batch(ocfg, 2, 42, ragged_text=True)
    img = torch.rand(2, 3, 384, 576, generator=g) * 2 - 1
    img[1, :, 352:, :] = 0                                                # sample 1: 11 x 18 valid patches
    batch["image"] = [img]
    p = dict(O.init_params(ocfg, 43), **M.mpp_init_params(ocfg, 44))
    masked, replaced = M.make_masks(img, ocfg, 45, "random")
    m = _module(ocfg, p, "bf16", long_sequences=True)
    xn, grads, _, dxn, mp, dpat, pb = _run_pass(m, batch, masked, replaced, 0.0)
    assert pb.d.L + 1 + pb.d.P == 257 and m.engine.stream_bit(pb.d) == L.MODE_STREAM_ATTN
    pp = {n_: (t.clone().requires_grad_(True) if n_ in PASS_GRADS else t) for n_, t in p.items()}
    out = M.infer_masked(pp, ocfg, batch["text_ids"], batch["text_masks"], img, replaced)
    im = out["image_masks"].bool()
    tol = PTOL["bf16"]
    assert float((xn[:, 40:][im] - out["image_feats"].detach()[im]).abs().max()) < tol["x"] * max(1.0, float(out["image_feats"].abs().max()))
    (out["image_feats"] * dxn[:, 40:]).sum().backward()
    for n_ in ("transformer.mask_token", "transformer.patch_embed.proj.bias"):
        want = pp[n_].grad
        assert float((grads[n_] - want).abs().max()) <= tol["grad"] * float(want.abs().max()) + 1e-8, n_


def test_visual_embed_mask_it_returns_the_reference_shapes():
    ocfg, p, batch = _pass_case("ragged")
    m = _module(ocfg, p, "f32")
    img = batch["image"][0]
    torch.manual_seed(5)
    emb, msk, (pi, hw), lab = m.visual_embed(img.to(DEV), mask_it=True)
    torch.manual_seed(5)
    masked = torch.bernoulli(torch.full((4, 12), 0.15)).bool()
    replaced = torch.bernoulli(torch.full((4, 12), 0.8)).bool() & masked
    assert tuple(lab.shape) == (4, 13, 3) and tuple(emb.shape) == (4, 13, 768) and hw == (3, 4)
    assert torch.equal(lab.cpu(), M.image_labels(img, ocfg, masked))
    x, mk = M.visual_embed_masked(p, img, ocfg, replaced)
    on = mk.bool()
    assert float((emb.cpu()[on] - x[on]).abs().max()) < 2e-3 * max(1.0, float(x.abs().max()))
    # the caller's masks replace the draw
    mk2, rp2 = M.make_masks(img, ocfg, 25, "ragged")
    emb2, _, _, lab2 = m.visual_embed(img.to(DEV), mask_it=True, mpp_masks=(mk2, rp2))
    assert torch.equal(lab2.cpu(), M.image_labels(img, ocfg, mk2))
    x2, _ = M.visual_embed_masked(p, img, ocfg, rp2)
    assert float((emb2.cpu()[on] - x2[on]).abs().max()) < 2e-3 * max(1.0, float(x2.abs().max()))
