"""-m gpu: rmcl_encoder_forward / _backward (and the _mpp forms, rmcl_visual_embed, rmcl_encoder_forward_rank) through the raw C ABI against
tests/encoder_ref.py in float64, block by block and row by row, at small shapes that leave D in {192, 768}: every mode, every embedding arm.

Metric.  Per row of each block, as tests/test_attention_kernels_gpu.py:
  err = |got - ref|_2 / max(|ref|_2, 0.05 * rms row norm of the block), asserted on the MAXIMUM over rows.
Blocks: the text rows and the image rows of xn ([CLS]-token rows only under RMCL_MODE_CLS_TAIL), dpatches, dtext, and every tensor of the
gradient arena (one block per tensor of runtime.param_specs; a matrix by rows, the position table by token, a vector as one row).
Bounds.  fp32 arms (dtype F32, exact 1): err <= 8 * max(e32, 2^-23), e32 = the same figure of encoder_ref run in fp32 torch on the CPU - summation
order, expf / erff / rsqrt only (factor and derivation of test_heads_kernels_gpu.py / test_wpa_kernels_gpu.py).  bf16 arms (exact 0):
err <= 3 * the figure of encoder_ref's rounding model (model = True, its docstring lists the rounding points) on the same case; 3 is BF16_FACTOR of
the attention pin, and tests/test_encoder_ref_cpu.py caps the model itself on the CPU.  Some blocks of a bf16 pass are computed in fp32 from fp32
inputs alone - the gradient of transformer.norm.bias is the column sum of dxn - and the model, fp32 torch, then shows only its own summation
order (6e-8 .. 8e-8 measured): such a block is held to the floor of the fp32 arms, 8 * 2^-23, the same arithmetic; a block the model leaves at
exactly 0 (a tensor without a gradient in the pass) must keep its bits.
The reference is computed on the values the kernel reads: the fp32 master arena (the model rounds the five weight matrices to bf16 once, like
the shadow arena) and, on the bf16 arms, bf16-valued patches.

Contract, every run: stash and workspace have exactly rmcl_stash_bytes / rmcl_workspace_bytes between 4 KiB guard zones of 0xA5, intact
afterwards; stash, workspace, xn, dpatches, dtext, pos_tok / dpos_tok start as NaN and every compared output is finite afterwards; co_mask
equals the reference mask; params, ids, masks, patches, dxn and the selection are unchanged; the gradient arena starts from non-zero values
(per tensor: noise of the rms of its reference gradient) and the pass adds to them - what it added, arena minus start, is the block compared -, elements between the tensors' slots keep their bits; DATA
mode passes grads32 = NULL; dpatches rows of replaced patches are exactly zero.

Cases (2 layers, vocab 64, patch_k 192 unless noted; weights as oracle.init_params scales them).  fp32 exact: A D 64 B 3 L 5 P 9 (one sample
with a single valid token, ids with 0 and duplicates, one all-zero patch) INFER / DATA / FULL; B D 320; C D 1024, 1 layer; D D 128 ragged
(grids 4x4 permuted, 1x4, 4x1, 2x3 of a 4x4 table); E token-type row 2 and the pair form; F the _mpp forms (replaced: none, some, all);
G cls_only 1 and RMCL_MODE_CLS_TAIL (FULL and DATA); H dropout 0.25 with the masks read back, dense and on the cls tail; I rmcl_visual_embed + the rank pass.  bf16: J D 128; K D 192
mlp 768 (rmcl_fold given under tune key 0 = 70 in INFER / DATA: tiled pre-activation, the fold is not taken there - the qkv GEMM, N = 576,
cannot run on the 192x384 kernel; the fold taken under key 0 = 60; FULL under key 70 without the fold); K2 D 384 mlp 768, the fold under key 0 = 60; L D 768 mlp 768 at M = 256 (grouped weight
gradients) and M = 192 (split-K); the cls tail on J (DATA) and on L at M = 256 (FULL: the tail layer beside the grouped launch).

Found by this file: the LayerNorm fold at D = 192 (test_K_bf16_layernorm_fold_taken_at_d192_under_key_60 has the cause and the fix).

RMCL_ENCODER_PARITY_OUT names a JSON file that receives every measured and allowed figure (profiles/encoder_parity.json is such a dump).
"""
import ctypes as C
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rmcl_oracle as O  # noqa: E402
from tests import encoder_ref as R  # noqa: E402
from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream, tdt  # noqa: E402

from tests.encoder_cases import (BF16_FACTOR, BF16_VARIANTS, F32_FACTOR, F32_FLOOR, MASK_TOKEN, MODES, REPLACED_A, SHAPES, allowance, blocks,  # noqa: E402,F401
                                 get_case, grad_start, keys_of, model_figures, pick, reference, row_err)

GUARD, GUARD_BYTE, NAN_BYTE = 4096, 0xA5, 0xFF       # 0xFF in every byte: NaN in fp32 and in bf16
PARITY = {}


def compare(label, c, got, dxn_kind, tail=False, G0=None, **extra):
    """Figures of every block against float64, the bound of the arm, the record, then the assertion."""
    if tail and c.bf16:                          # the yardstick follows the kernel's tail: fp32 behind the last attention (encoder_ref tail = True)
        extra = dict(extra, tail=True)
    ref = blocks(c, pick(reference(c.name, "f64", dxn_kind, **extra), got), None, tail)
    yard = blocks(c, pick(reference(c.name, "model" if c.bf16 else "f32", dxn_kind, **extra), got), G0, tail)
    mine = blocks(c, got, G0, tail, added=True)
    assert set(mine) == set(ref), (sorted(mine), sorted(ref))
    rec, bad = {}, []
    for b in sorted(ref):
        assert bool(torch.isfinite(mine[b].float()).all()), f"{label}: {b} is not finite"
        e, y = row_err(mine[b], ref[b]), row_err(yard[b], ref[b])
        allowed = allowance(c.bf16, y)
        rec[b] = {"kernel": e, "model" if c.bf16 else "e32": y, "allowed": allowed}
        if b.startswith("G:") and not bool(ref[b].any()):
            assert not bool(mine[b].any()), f"{label}: {b} has no gradient in this pass and was written"
        if not e <= allowed:
            bad.append(f"{b}: {e:.3e} > {allowed:.3e}")
    PARITY[label] = rec
    worst = max(rec.items(), key=lambda kv: kv[1]["kernel"] / kv[1]["allowed"] if kv[1]["allowed"] else 0.0)
    print(f"{label}: worst block {worst[0]} kernel {worst[1]['kernel']:.3e} allowed {worst[1]['allowed']:.3e}")
    assert not bad, f"{label}: " + "; ".join(bad)


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_ENCODER_PARITY_OUT")
    if out and PARITY:
        from tests.encoder_cases import MODEL_CAPS
        for label, rec in PARITY.items():
            caps = MODEL_CAPS.get(label)
            for b, v in rec.items():
                if caps and "model" in v:
                    v["model_cpu_cap"] = caps[b]
        ratio = lambda v: v["kernel"] / v["allowed"] if v["allowed"] else 0.0
        worst = max((ratio(v), f"{label}:{b}") for label, rec in PARITY.items() for b, v in rec.items())
        head = {"metric": "worst row of |got - ref|_2 / max(|ref|_2, 0.05 rms row norm), against encoder_ref in float64",
                "allowed": "fp32 arms 8 * max(e32, 2^-23); bf16 arms 3 * model", "largest_kernel_over_allowed": worst[0], "largest_at": worst[1]}
        with open(out, "w") as f:                  # one line per block
            f.write("{" + ", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in head.items()) + ',\n "cases": {\n')
            f.write(",\n".join(f"  {json.dumps(label)}: {{\n" + ",\n".join(f"   {json.dumps(b)}: {json.dumps(v, sort_keys=True)}" for b, v in sorted(rec.items()))
                                + "}" for label, rec in sorted(PARITY.items())))
            f.write("}}\n")


# ------------------------------------------------------------------------------------------ device side
class Guarded:
    """A device buffer of exactly `nbytes` bytes, every byte 0xFF (NaN in fp32 and in bf16), between two guard zones."""

    def __init__(self, nbytes):
        self.raw = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + nbytes]
        self.t.fill_(NAN_BYTE)
        self.nbytes = nbytes

    def intact(self):
        return bool((self.raw[:GUARD] == GUARD_BYTE).all()) and bool((self.raw[GUARD + self.nbytes:] == GUARD_BYTE).all())


def bits(t):
    return t.contiguous().view(torch.uint8)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


class Keys:
    """rmcl_tune_set pairs for a region, restored on the way out (process-global)."""
    DEFAULTS = {0: -1}

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            check(lib.rmcl_tune_set(k, v), "tune_set")

    def __exit__(self, *exc):
        for k in self.kv:
            check(lib.rmcl_tune_set(k, self.DEFAULTS[k]), "tune_set")


def run(c, mode, G0=None, dxn=None, tail=False, cls_only=0, fold=False, lpT=False, replaced=None, drop_p=0.0, seed=1234, masks_of=None,
        expect_tiled=False):
    """One forward (+ backward unless INFER) through the C ABI under the contract of the docstring.  Returns CPU tensors."""
    d, cd, dt = c.dims, c.cd, c.dims.dtype
    B, N, D, Pn, Lt = d.B, c.N, d.D, d.P, d.L
    M = B * N
    p32 = c.arena.to(DEV)
    plp = p32.bfloat16() if c.bf16 else None
    plpT = None
    if lpT:
        plpT = torch.zeros_like(plp)
        check(lib.rmcl_weight_transpose_bf16(C.byref(cd), P(plp), P(plpT), stream()), "weight_transpose")
    fo = None
    keep_alive = []
    if fold:
        wf = torch.zeros(int(lib.rmcl_ln_fold_elems(C.byref(cd), 0)), dtype=torch.bfloat16, device=DEV)
        sc = torch.zeros(int(lib.rmcl_ln_fold_elems(C.byref(cd), 1)), dtype=torch.float32, device=DEV)
        check(lib.rmcl_ln_fold(C.byref(cd), P(p32), P(wf), P(sc), stream()), "ln_fold")
        fo = L.Fold(wf.data_ptr(), sc.data_ptr())
        keep_alive += [wf, sc]
    ids, tm = c.text_ids.to(DEV), c.text_mask.to(DEV)
    pat = c.patches.to(DEV, tdt(dt))
    inputs = [p32, ids, tm, pat] + ([plp] if c.bf16 else []) + ([plpT] if lpT else [])
    rg = None
    pos_tok = dpos_tok = None
    if c.ragged:
        sel, cnt, hw = (c.ragged[k].to(DEV) for k in ("sel", "counts", "hw"))
        pos_tok, dpos_tok = nan(B, Pn + 1, D), nan(B, Pn + 1, D)
        rg = L.Ragged(sel.data_ptr(), cnt.data_ptr(), hw.data_ptr(), Pn, c.ragged["gw"], c.ragged["G0"], pos_tok.data_ptr(), dpos_tok.data_ptr())
        inputs += [sel, cnt, hw]
    rep = None
    if replaced is not None:
        rep = torch.tensor(replaced, dtype=torch.int32).to(DEV)
        inputs.append(rep)
    mt_off = c.offs[MASK_TOKEN][0]
    dxn_d = None if dxn is None else dxn.to(DEV).contiguous()
    if dxn_d is not None:
        inputs.append(dxn_d)
    before = [t.clone() for t in inputs]
    base = mode
    stash = Guarded(int(lib.rmcl_stash_bytes(C.byref(cd), base)))
    ws = Guarded(int(lib.rmcl_workspace_bytes(C.byref(cd))))
    xn = nan(M, D)
    co = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    sd, dp = C.c_uint32(seed), C.c_float(drop_p)
    rgp, fop = (C.byref(rg) if rg else None), (C.byref(fo) if fo else None)
    fmode = mode | (L.MODE_CLS_TAIL if tail else 0)
    if replaced is not None:
        check(lib.rmcl_encoder_forward_mpp(C.byref(cd), fmode, P(p32), P(plp), P(ids), P(tm), P(pat), P(co), P(stash.t), P(ws.t), P(xn), sd, dp, rgp, fop,
                                           P(rep), I64(mt_off), stream()), "encoder_forward_mpp")
    else:
        check(lib.rmcl_encoder_forward(C.byref(cd), fmode, P(p32), P(plp), P(ids), P(tm), P(pat), P(co), P(stash.t), P(ws.t), P(xn), sd, dp, rgp, fop,
                                       stream()), "encoder_forward")
    out = {}
    G = None
    if mode != L.MODE_INFER:
        out_dp, out_dt = nan(B * Pn, d.patch_k, dtype=tdt(dt)), nan(B * Lt, D)
        if mode == L.MODE_FULL:
            G = G0.to(DEV)
        args = [C.byref(cd), mode, P(p32), P(plp), P(ids), P(pat), P(co), P(stash.t), P(ws.t), P(dxn_d)]
        rest = [P(out_dp), P(out_dt), P(G), sd, dp, rgp, P(plpT)]
        if replaced is not None:
            check(lib.rmcl_encoder_backward_mpp(*args, *rest, P(rep), I64(mt_off), stream()), "encoder_backward_mpp")
        else:
            check(lib.rmcl_encoder_backward(*args, cls_only, *rest, stream()), "encoder_backward")
        if expect_tiled:
            # the forward took the tiled pre-activation stash: a backward without the transposed shadows is refused before any launch
            rc = lib.rmcl_encoder_backward(*args, cls_only, *rest[:-1], None, stream())
            assert rc != 0 and b"tiled" in lib.rmcl_last_error(), "the forward did not take the tiled pre-activation stash"
        out.update(dpatches=out_dp, dtext=out_dt)
    torch.cuda.synchronize()
    assert stash.intact(), "stash: guard bytes overwritten"
    assert ws.intact(), "workspace: guard bytes overwritten"
    for a, b in zip(inputs, before):
        assert torch.equal(bits(a), bits(b)), "an input was modified"
    res = {"xn": xn.cpu().view(B, N, D), "co": co.cpu()}
    for k, v in out.items():
        res[k] = v.float().cpu()
    if G is not None:
        res["G"] = G.cpu()
        covered = torch.zeros(c.total, dtype=torch.bool)
        for name, off, shape in c.specs:
            covered[off:off + R.numel(shape)] = True
        assert torch.equal(res["G"][~covered], G0[~covered]), "the pass wrote between the tensors of the gradient arena"
    if c.ragged:
        res["pos_tok"] = pos_tok.cpu()
    if masks_of:
        def mask(shape, layer, site):
            x = torch.ones(shape, device=DEV)
            check(lib.rmcl_dropout_mask_apply(P(x), I64(x.numel()), sd, layer, site, dp, stream()), "dropout_mask_apply")
            return x.cpu()
        drop = {"text": mask((B, Lt, D), 0, 3), "image": mask((B, Pn + 1, D), 0, 4)}
        for l in range(d.layers):
            drop[l] = {"proj": mask((B, N, D), l, 0), "hidden": mask((B, N, d.mlp), l, 1), "fc2": mask((B, N, D), l, 2)}
        res["drop"] = drop
    del keep_alive
    return res


def check_pass(label, c, mode, dxn_kind="full", tail=False, cls_only=0, **kw):
    """run() + co_mask + compare() for a case whose reference needs nothing from the device."""
    extra = {}
    if kw.get("replaced") is not None:
        extra.update(replaced=kw["replaced"], mask_token=MASK_TOKEN)
    if kw.get("fold"):
        extra.update(fold=True)
    if kw.pop("pass_fold", False):               # the pair is handed over, the pass is expected NOT to take the fold: plain model
        kw["fold"] = True
    dk = None if mode == L.MODE_INFER else dxn_kind
    ref = reference(c.name, "f64", dk, **extra)
    G0 = grad_start(c, ref) if mode == L.MODE_FULL else None
    dxn = None
    if dk:
        dxn = (c.dxn if dxn_kind == "full" else c.dxn_cls).reshape(-1, c.dims.D)
        if cls_only:
            dxn = c.dxn[:, 0]
    got = run(c, mode, G0=G0, dxn=dxn, tail=tail, cls_only=cls_only, **kw)
    assert torch.equal(got["co"], ref["co"]), f"{label}: co_mask differs from the reference mask"
    if kw.get("replaced") is not None and "dpatches" in got:
        rows = torch.tensor(kw["replaced"]).flatten().bool()
        assert rows.any() and not bool(got["dpatches"][rows].any()), f"{label}: dpatches of a replaced patch is not exactly zero"
    compare(label, c, pick(got, keys_of(mode)), dk, tail=tail, G0=G0, **extra)
    return got


# ------------------------------------------------------------------------------------------ fp32 exact arms
@pytest.mark.parametrize("mode", ["infer", "data", "full"])
def test_A_d64_partial_blocks_pad_id_colliding_ids(mode):
    check_pass(f"A:{mode}", get_case("A"), MODES[mode])


def test_B_d320_second_column_block():
    check_pass("B:full", get_case("B"), L.MODE_FULL)


def test_C_d1024_upper_limit():
    check_pass("C:full", get_case("C"), L.MODE_FULL)


def test_D_ragged_position_resize_and_pad_slots():
    c = get_case("D")
    assert any(1 in tuple(int(v) for v in hw) for hw in c.ragged["hw"]) and int(c.ragged["counts"].min()) < c.dims.P
    got = check_pass("D:full", c, L.MODE_FULL)
    tab = R.views(c.arena, c.specs)["transformer.pos_embed"][0]
    want, y32 = (R._pos_rows(tab.to(t), c.ragged, c.dims.B, c.dims.P, c.dims.D).reshape(-1, c.dims.D) for t in (torch.float64, torch.float32))
    e, y = row_err(got["pos_tok"].reshape(-1, c.dims.D), want), row_err(y32, want)
    PARITY["D:pos_tok"] = {"pos_tok": {"kernel": e, "e32": y, "allowed": F32_FACTOR * max(y, F32_FLOOR)}}
    assert e <= F32_FACTOR * max(y, F32_FLOOR), (e, y)


def test_E_token_type_row_2():
    check_pass("E:img_type2", get_case("E2"), L.MODE_FULL)


def test_E_token_type_pair_form():
    check_pass("E:pair", get_case("Ep"), L.MODE_FULL)


@pytest.mark.parametrize("mode", ["data", "full"])
def test_F_mask_token_substitution(mode):
    check_pass(f"F:{mode}", get_case("A"), MODES[mode], replaced=REPLACED_A)


def test_G_cls_only_on_a_dense_stash():
    check_pass("G:cls_only1", get_case("A"), L.MODE_FULL, dxn_kind="cls", cls_only=1)


def test_G_cls_tail():
    check_pass("G:cls_tail", get_case("A"), L.MODE_FULL, dxn_kind="cls", tail=True, cls_only=2)


def test_G_cls_tail_data_mode():
    check_pass("G:cls_tail:data", get_case("A"), L.MODE_DATA, dxn_kind="cls", tail=True, cls_only=2)


def _dropout_full_pass(label, tail):
    """Case A, FULL, dropout 0.25 against the reference with the masks the library reports.  tail: the forward with RMCL_MODE_CLS_TAIL and the
    backward with cls_only = 2 - the compact rows draw the dense rows' masks, so the reference is the dense one with the cls-only dxn."""
    c = get_case("A")
    dry = run(c, L.MODE_INFER, drop_p=0.25, masks_of=True)             # the masks are a pure function of (seed, site, element)
    drop = dry["drop"]
    assert any(bool((m == 0).any()) for m in (drop["text"], drop["image"], drop[0]["proj"], drop[1]["hidden"], drop[1]["fc2"]))
    kw = dict(ragged=None, img_of=None, drop=drop)
    dxn = c.dxn_cls if tail else c.dxn
    ref = R.grads(c.arena, c.specs, c.dims, c.text_ids, c.text_mask, c.patches, dxn, torch.float64, **kw)
    y32 = R.grads(c.arena, c.specs, c.dims, c.text_ids, c.text_mask, c.patches, dxn, torch.float32, **kw)
    G0 = grad_start(c, ref)
    if tail:
        got = run(c, L.MODE_FULL, G0=G0, dxn=c.dxn[:, 0], tail=True, cls_only=2, drop_p=0.25)
    else:
        got = run(c, L.MODE_FULL, G0=G0, dxn=c.dxn.reshape(-1, c.dims.D), drop_p=0.25)
    assert torch.equal(got["co"], ref["co"])
    rb, yb = blocks(c, ref, None, tail), blocks(c, y32, G0, tail)
    mb = blocks(c, {k: got[k] for k in ("xn", "dpatches", "dtext", "G")}, G0, tail, added=True)
    rec, bad = {}, []
    for b in sorted(rb):
        assert bool(torch.isfinite(mb[b]).all()), b
        e, y = row_err(mb[b], rb[b]), row_err(yb[b], rb[b])
        rec[b] = {"kernel": e, "e32": y, "allowed": F32_FACTOR * max(y, F32_FLOOR)}
        if not e <= rec[b]["allowed"]:
            bad.append(f"{b}: {e:.3e} > {rec[b]['allowed']:.3e}")
    PARITY[label] = rec
    assert not bad, "; ".join(bad)


def test_H_dropout_with_the_masks_read_back():
    _dropout_full_pass("H:dropout", tail=False)


def test_H_dropout_on_the_cls_tail():
    _dropout_full_pass("H:dropout:cls_tail", tail=True)


def run_rank(c):
    """rmcl_visual_embed into a cache, then the rank pass over it, under the contract of the docstring.  Returns CPU tensors."""
    d, cd = c.dims, c.cd
    B, Pn, D, Lt, N, Bt = d.B, d.P, d.D, d.L, c.N, c.Bt
    ld_tok = Pn + 4
    p32 = c.arena.to(DEV)
    pat = c.patches.to(DEV)
    sel, cnt, hw = (c.ragged[k].to(DEV) for k in ("sel", "counts", "hw"))
    pos_tok = nan(B, Pn + 1, D)
    rg = L.Ragged(sel.data_ptr(), cnt.data_ptr(), hw.data_ptr(), Pn, 4, 4, pos_tok.data_ptr(), None)
    ws = Guarded(int(lib.rmcl_workspace_bytes(C.byref(cd))))
    emb, msk = nan(B, Pn + 1, D), torch.full((B, Pn + 1), -7, dtype=torch.int32, device=DEV)
    check(lib.rmcl_visual_embed(C.byref(cd), P(p32), None, P(pat), C.byref(rg), P(ws.t), P(emb), P(msk), stream()), "visual_embed")
    cache, cmask = torch.zeros(B, ld_tok, D, device=DEV), torch.zeros(B, ld_tok, dtype=torch.int32, device=DEV)
    cache[:, :Pn + 1], cmask[:, :Pn + 1] = emb, msk
    # the rank pass: Bt captions, each with the cached image img_of names (one name is outside the cache)
    dr = L.Dims(**{**vars(d), "B": Bt})
    ids, tm = c.text_ids.to(DEV), c.text_mask.to(DEV)
    img_of = torch.tensor(c.rank, dtype=torch.int32).to(DEV)
    assert any(not 0 <= i < B for i in c.rank)
    src = L.RankSrc(cache.data_ptr(), cmask.data_ptr(), img_of.data_ptr(), B, ld_tok)
    ws2 = Guarded(int(lib.rmcl_workspace_bytes(C.byref(dr))))
    xn, co = nan(Bt * N, D), torch.full((Bt, N), -7, dtype=torch.int32, device=DEV)
    keep = [t.clone() for t in (p32, pat, cache, cmask, ids, tm, img_of)]
    check(lib.rmcl_encoder_forward_rank(C.byref(dr), L.MODE_INFER, P(p32), None, P(ids), P(tm), C.byref(src), P(co), P(ws2.t), P(xn), None, stream()),
          "encoder_forward_rank")
    torch.cuda.synchronize()
    assert ws.intact() and ws2.intact()
    for a, b in zip((p32, pat, cache, cmask, ids, tm, img_of), keep):
        assert torch.equal(bits(a), bits(b))
    assert bool(torch.isfinite(emb).all())
    return {"emb": emb.cpu(), "msk": msk.cpu(), "xn": xn.cpu().view(Bt, N, D), "co": co.cpu()}


def test_I_visual_embed_cache_and_rank_pass():
    c = get_case("I")
    d = c.dims
    B, D, Lt = d.B, d.D, d.L
    got = run_rank(c)
    emb, msk, xn, co = got["emb"], got["msk"], got["xn"], got["co"]
    parts = {}
    R.encoder_ref(c.arena.double(), c.specs, d, c.text_ids, c.text_mask, c.patches.double(), ragged=c.ragged, img_of=c.rank, parts=parts)
    p32_parts = {}
    R.encoder_ref(c.arena, c.specs, d, c.text_ids, c.text_mask, c.patches, ragged=c.ragged, img_of=c.rank, parts=p32_parts)
    assert torch.equal(msk, parts["visual_mask"])
    e = row_err(emb.reshape(-1, D), parts["visual"].reshape(-1, D))
    y = row_err(p32_parts["visual"].reshape(-1, D), parts["visual"].reshape(-1, D))
    PARITY["I:visual_embed"] = {"visual": {"kernel": e, "e32": y, "allowed": F32_FACTOR * max(y, F32_FLOOR)}}
    assert e <= F32_FACTOR * max(y, F32_FLOOR), (e, y)
    ref = reference("I", "f64", None)
    assert torch.equal(co, ref["co"])
    missing = [b for b, i in enumerate(c.rank) if not 0 <= i < B]
    assert not bool(co[missing, Lt:].any())
    compare("I:rank", c, {"xn": xn}, None)


# ------------------------------------------------------------------------------------------ bf16 arms
@pytest.mark.parametrize("mode", ["data", "full"])
def test_J_bf16_generic_small_route(mode):
    check_pass(f"J:{mode}", get_case("J"), MODES[mode])


def test_J_bf16_cls_tail_data_mode():
    """The bf16 cls-row gather (or the in-place bf16 read of the streaming skinny kernel) and the scatter-cast of d(attention output)."""
    check_pass("J:cls_tail:data", get_case("J"), L.MODE_DATA, dxn_kind="cls", tail=True, cls_only=2)


def _same_xn(a, b):
    return torch.equal(a["xn"].view(torch.int32), b["xn"].view(torch.int32))


@pytest.mark.parametrize("mode", ["infer", "data"])
def test_K_bf16_fold_given_under_key_70_tiled_preactivation(mode):
    """rmcl_fold given under tune key 0 = 70.  The fold is taken only where all four GEMMs of a layer run on the 192-row tile kernels
    (encoder_forward_impl); with key 0 = 70 the qkv GEMM of this shape (N = 576, no multiple of 384) does not, so the pass runs the separate
    LayerNorm kernels - bit for bit the pass without the pair - and, in DATA mode, stashes the MLP pre-activation in tile order."""
    c = get_case("K")
    with Keys(k0=70):
        # the MLP GEMMs of this encoder go to the 192x384 kernel, the only one with the tiled stash
        assert lib.rmcl_gemm_route(c.dims.B * c.N, c.dims.mlp, c.dims.D, L.EPI_BIAS | L.EPI_GELU | L.EPI_SAVE_PREACT, L.BF16, 1, 1) == 2
        got = check_pass(f"K:{mode}:fold_given", c, MODES[mode], lpT=mode == "data", expect_tiled=mode == "data", pass_fold=True)
        if mode == "infer":
            assert _same_xn(got, run(c, L.MODE_INFER)), "the fold was taken although the qkv GEMM cannot run on a 192-row tile kernel"


@pytest.mark.parametrize("mode", ["infer", "data"])
def test_K_bf16_layernorm_fold_taken_at_d192_under_key_60(mode):
    """D = 192 under tune key 0 = 60, which sends every GEMM the 192x192 kernel supports there: the fold IS taken (the bits of xn differ from
    the pass without the pair) and is held to the model with the fold's own roundings (encoder_ref fold = True).
    This case found a bug: the pass took the fold and computed garbage (worst-row error 1.07 from a zeroed workspace, NaN from a NaN one).
    rmcl_launch_gemm asked rmcl_gemm_fast_supported - the 128x128 kernel's rule, N % 128 == 0 - before the router, so a GEMM with N = D = 192
    or 3 D = 576 went to the exact kernels, which dropped EPI_ROWSTAT / EPI_LNFOLD without a word: the producer's bf16 copy and row partials
    were never written.  Fixed in csrc/gemm_fast.hip (rmcl_gemm_fast_takes: such a GEMM stays on the bf16 path when the router sends it to a
    192-row tile kernel; rmcl_gemm_routes_to_tile192 and the tiled-stash decision ask it too) and csrc/api.cpp (rmcl_launch_gemm refuses a
    folded epilogue it would hand to the exact kernels)."""
    c = get_case("K")
    with Keys(k0=60):
        got = check_pass(f"K:{mode}:fold60", c, MODES[mode], fold=True, lpT=mode == "data")
        if mode == "infer":
            assert not _same_xn(got, run(c, L.MODE_INFER)), "the pass with rmcl_fold given did not take the folded GEMMs"


@pytest.mark.parametrize("mode", ["infer", "data"])
def test_K2_bf16_layernorm_fold_taken_at_d384_under_key_60(mode):
    """D = 384 (a multiple of 192 AND of 128: every GEMM is one the 128x128 kernel could take too) under tune key 0 = 60: all four GEMMs
    of a layer run on the 192x192 kernel, the fold IS taken (the bits of xn differ from the pass without the pair) and is held to the model
    with the fold's own roundings (encoder_ref fold = True)."""
    c = get_case("K2")
    with Keys(k0=60):
        got = check_pass(f"K2:{mode}:fold60", c, MODES[mode], fold=True, lpT=mode == "data")
        if mode == "infer":
            assert not _same_xn(got, run(c, L.MODE_INFER)), "the pass with rmcl_fold given did not take the folded GEMMs"


def test_K_bf16_full_without_the_fold():
    with Keys(k0=70):
        check_pass("K:full", get_case("K"), L.MODE_FULL, lpT=True, expect_tiled=True)


@pytest.mark.parametrize("name", ["L4", "L3"])
def test_L_bf16_d768_grouped_and_split_k_weight_gradients(name):
    c = get_case(name)
    M = c.dims.B * c.N
    assert (M % 64 == 0 and M >= 256) == (name == "L4")
    check_pass(f"{name}:full", c, L.MODE_FULL, lpT=True)


def test_L4_bf16_cls_tail_with_grouped_weight_gradients():
    """M = 256: the grouped weight-gradient launch for the first layer; the tail layer forms fc2 / fc1 / proj gradients from the B cls rows and
    only its qkv gradient reduces over all tokens (encoder_backward_impl, the grouped branch of the tail layer)."""
    check_pass("L4:cls_tail:full", get_case("L4"), L.MODE_FULL, dxn_kind="cls", tail=True, cls_only=2, lpT=True)
