"""-m gpu: sequences of 257..512 tokens on the bf16 path - RMCL_MODE_STREAM_ATTN through the encoder's C ABI, and config["long_sequences"]
through the engine, the fine-tuning tasks and the recall evaluation.  2 layers, seed-initialised weights, drop_rate = 0 throughout.

Encoder.  L = 40, P = 240 (N = 281: a 384 x 640 image), B = 2, bf16, FULL mode, the same inputs with and without the mode bit.  Without
it the attention is the unfused path (score / probability matrices), which is the yardstick; with it the streaming kernels run.  Compared:
xn, dpatches, dtext and every tensor of the gradient arena, under the bf16 bounds tests/test_parity2_gpu.py applies to the same
quantities of a zero-padded batch (test_bf16_ragged_images_track_reference_golden): cls rows 3e-2 and token features 0.1 absolute (features
are O(1..4) behind the final LayerNorm), gradients 0.12 relative - applied here to |a - b| / |b| of each whole tensor, which is stricter than
that test's comparison of norms.  At P = 144 (185 tokens) the bit changes no bit of any output: every output of a DATA-mode pass and
every output in front of the gradient arena in FULL mode (the arena's atomic split-K sums are not reproducible run to run - see the test).  A backward whose bit differs from its
forward's is refused (-1) at 281 tokens.

Engine.  long_sequences = True on a bf16 engine against the fp32 engine (pinned to the reference, no token limit) on the same weights and
the same zero-padded batch of a 384 x 640, a 384 x 576 and a 320 x 384 image (281 tokens): a VQA step, an NLVR2 pair step, an itm + irtr
step and one attacked VQA step (K = 2).  Bounds: TOL["bf16"] of tests/test_vqa_gpu.py / test_nlvr2_gpu.py / test_irtr_gpu.py, the class
the bf16 task tests apply at <= 256 tokens: loss 1e-2 relative, every parameter's gradient norm 0.1 relative (+ 2e-7), logits 0.1 * max(1, max |reference|), and
element-wise 0.1 * 2.5 * max |reference| on the whole pooler, first qkv and head weight gradients (the rule those tests apply to slices);
the patch gradient of the first PGD step falls under both gradient rules.

Recall.  The scenario of tests/test_irtr_gpu.py test_over_long_image_is_refused_before_any_scoring (image 6 at 384 x 576: 257 tokens):
a [10, 10] finite score matrix within TOL["bf16"]["logits"] (relative to max(1, max |score|), as test_recall_bf16_scores_in_class) of the
fp32 engine's.  Under the default config the same calls still raise, and 513 tokens raise under long_sequences too."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P  # noqa: E402
from rmcl_amd.runtime import stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import objectives  # noqa: E402
from tests import irtr_oracle as R  # noqa: E402
from tests import nlvr2_oracle as N  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402
from tests.test_irtr_gpu import TOL as TOL_IRTR, make_module as make_irtr_module, _run as run_irtr  # noqa: E402
from tests.test_nlvr2_gpu import TOL as TOL_NLVR2, make_module as make_nlvr2_module, _run as run_nlvr2  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402
from tests.test_vqa_gpu import TOL as TOL_VQA, make_vqa_module, _step as vqa_step  # noqa: E402

DEV = "cuda:0"
SIZES = [(384, 640), (384, 576), (320, 384)]                 # 240, 216 and 120 patches: 281 tokens
# tests/test_parity2_gpu.py test_bf16_ragged_images_track_reference_golden: e_cls < 3e-2, e_img < 0.1, gradient norms within 0.12
CLS_TOL, FEAT_TOL, GRAD_TOL = 3e-2, 0.1, 0.12


# ---- encoder, C ABI -------------------------------------------------------------------------------------------------------------
class EncoderCase:
    def __init__(self, Pn, B=2, Lt=40, layers=2):
        self.d = d = L.Dims(B=B, L=Lt, P=Pn, D=768, H=12, layers=layers, mlp=3072, patch_k=3072, proj=128, vocab=128, dtype=L.BF16, exact=0,
                            Pp=Pn, n_types=0, img_type=0)
        self.lay = lay = L.Layout()
        lib.rmcl_param_layout(C.byref(d), C.byref(lay))
        g = torch.Generator().manual_seed(11 + Pn)
        p = torch.randn(int(lay.total), generator=g) * 0.02
        for off in [lay.eln_w, lay.norm_w] + [lay.layer0 + l * lay.layer_stride + o for l in range(layers) for o in (lay.ln1_w, lay.ln2_w)]:
            p[off:off + d.D] += 1.0
        self.p32 = p.to(DEV)
        self.plp = self.p32.bfloat16()
        self.N = N_ = Lt + 1 + Pn
        self.text_ids = torch.randint(0, 128, (B, Lt), generator=g).to(DEV)
        tm = torch.ones(B, Lt, dtype=torch.int64)
        tm[0, 23:] = 0
        tm[1, 9:] = 0
        self.text_mask = tm.to(DEV)
        pat = torch.randn(B * Pn, d.patch_k, generator=g)
        pat[(B - 1) * Pn + Pn - 24:] = 0                       # the last sample's last 24 patches are padding (masked image tokens)
        self.patches = pat.to(DEV).bfloat16()
        self.dxn = torch.randn(B * N_, d.D, generator=g).to(DEV)
        self.stash = torch.empty(int(lib.rmcl_stash_bytes(C.byref(d), L.MODE_FULL)), dtype=torch.uint8, device=DEV)
        assert self.stash.numel() == int(lib.rmcl_stash_bytes(C.byref(d), L.MODE_FULL | L.MODE_STREAM_ATTN))   # the bit does not resize the stash
        self.ws = torch.empty(int(lib.rmcl_workspace_bytes(C.byref(d))), dtype=torch.uint8, device=DEV)

    def forward(self, bit, mode=L.MODE_FULL):
        d = self.d
        co = torch.zeros(d.B, self.N, dtype=torch.int32, device=DEV)
        xn = torch.zeros(d.B * self.N, d.D, device=DEV)
        check(lib.rmcl_encoder_forward(C.byref(d), mode | bit, P(self.p32), P(self.plp), P(self.text_ids), P(self.text_mask),
                                       P(self.patches), P(co), P(self.stash), P(self.ws), P(xn), C.c_uint32(0), C.c_float(0.0), None, None,
                                       stream_ptr()), "encoder_forward")
        return co, xn

    def backward_rc(self, bit, co, out, mode=L.MODE_FULL):
        d = self.d
        return lib.rmcl_encoder_backward(C.byref(d), mode | bit, P(self.p32), P(self.plp), P(self.text_ids), P(self.patches), P(co),
                                         P(self.stash), P(self.ws), P(self.dxn), 0, P(out["dpatches"]), P(out["dtext"]), P(out.get("G")),
                                         C.c_uint32(0), C.c_float(0.0), None, None, stream_ptr())

    def run(self, bit, mode=L.MODE_FULL):
        d = self.d
        co, xn = self.forward(bit, mode)
        out = {"dpatches": torch.zeros(d.B * d.P, d.patch_k, dtype=torch.bfloat16, device=DEV), "dtext": torch.zeros(d.B * d.L, d.D, device=DEV)}
        if mode == L.MODE_FULL:
            out["G"] = torch.zeros(int(self.lay.total), device=DEV)
        check(self.backward_rc(bit, co, out, mode), "encoder_backward")
        torch.cuda.synchronize()
        out.update(xn=xn, co=co)
        return out


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def test_encoder_mode_bit_at_281_tokens_tracks_the_unfused_path():
    ec = EncoderCase(240)
    ref, got = ec.run(0), ec.run(L.MODE_STREAM_ATTN)
    assert torch.equal(ref["co"], got["co"]) and int((ref["co"] == 0).sum()) == 17 + 31 + 24
    N_ = ec.N
    dx = (got["xn"] - ref["xn"]).abs().view(ec.d.B, N_, -1)
    valid = ref["co"].bool()
    e_cls, e_tok = float(dx[:, 0].max()), float(dx[valid].max())
    print(f"xn: cls rows max |d| {e_cls:.3e}, valid tokens max |d| {e_tok:.3e} (max |xn| {float(ref['xn'].abs().max()):.2f})")
    assert e_cls < CLS_TOL and e_tok < FEAT_TOL, (e_cls, e_tok)
    assert torch.isfinite(got["xn"]).all() and torch.isfinite(got["G"]).all()
    worst = {}
    for k in ("dpatches", "dtext"):
        worst[k] = rel(got[k], ref[k])
    lay, d = ec.lay, ec.d
    names = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
    sizes = dict(ln1_w=d.D, ln1_b=d.D, qkv_w=3 * d.D * d.D, qkv_b=3 * d.D, proj_w=d.D * d.D, proj_b=d.D, ln2_w=d.D, ln2_b=d.D,
                 fc1_w=d.mlp * d.D, fc1_b=d.mlp, fc2_w=d.mlp * d.D, fc2_b=d.D)
    for l in range(d.layers):
        for n in names:
            o = lay.layer0 + l * lay.layer_stride + getattr(lay, n)
            worst[f"layer{l}.{n}"] = rel(got["G"][o:o + sizes[n]], ref["G"][o:o + sizes[n]])
    for n, o, sz in (("word", lay.word, d.vocab * d.D), ("pos", lay.pos, d.L * d.D), ("cls", lay.cls, d.D), ("pos_img", lay.pos_img, (d.P + 1) * d.D),
                     ("patch_w", lay.patch_w, d.D * d.patch_k), ("patch_b", lay.patch_b, d.D), ("norm_w", lay.norm_w, d.D), ("norm_b", lay.norm_b, d.D)):
        assert float(ref["G"][o:o + sz].norm()) > 0, n
        worst[n] = rel(got["G"][o:o + sz], ref["G"][o:o + sz])
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("largest |a - b| / |b|:", ", ".join(f"{k} {v:.3e}" for k, v in top))
    assert top[0][1] < GRAD_TOL, top
    assert rel(got["G"], ref["G"]) < GRAD_TOL
    # the streaming path is not the unfused one in disguise: the `probs` stash differs, so some bits do
    assert not torch.equal(got["xn"], ref["xn"])


def test_encoder_mode_bit_changes_nothing_at_185_tokens():
    """DATA mode (the PGD passes: every output is reproducible run to run) carries the claim without a condition: xn, the mask, dpatches and
    dtext - the end of the whole backward chain, attention included - are the same bits with and without the bit.  FULL mode adds the
    gradient arena, whose weight gradients are split-K sums through fp32 atomics (not reproducible run to run with or without the bit):
    there the outputs in front of the arena are compared bit for bit, and the arena bit for bit whenever two runs WITHOUT the bit agree."""
    ec = EncoderCase(144)
    d0, d1, d2 = ec.run(0, L.MODE_DATA), ec.run(0, L.MODE_DATA), ec.run(L.MODE_STREAM_ATTN, L.MODE_DATA)
    for k in ("xn", "co", "dpatches", "dtext"):
        assert torch.equal(d0[k].view(torch.uint8), d1[k].view(torch.uint8)), ("DATA mode is not reproducible", k)
        assert torch.equal(d0[k].view(torch.uint8), d2[k].view(torch.uint8)), ("DATA", k)
    assert float(d0["dpatches"].float().abs().max()) > 0
    a, a2, b = ec.run(0), ec.run(0), ec.run(L.MODE_STREAM_ATTN)
    for k in ("xn", "co", "dpatches", "dtext"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), ("FULL", k)
    repro = torch.equal(a["G"].view(torch.uint8), a2["G"].view(torch.uint8))
    print(f"gradient arena: two runs without the bit bit-identical: {repro}; |a2 - a| / |a| {rel(a2['G'], a['G']):.3e}, "
          f"with the bit |b - a| / |a| {rel(b['G'], a['G']):.3e}")
    if repro:
        assert torch.equal(a["G"].view(torch.uint8), b["G"].view(torch.uint8)), "G"
    else:
        # not the bit-for-bit claim (DATA mode above is): a coarse guard against a different computation.  The weight-gradient launches
        # read the stash and the dX chain, both shown bit-identical above, so only the order of the atomic adds can differ; a reordered
        # fp32 sum of the 370 rows a weight gradient adds up moves it by parts in 2^24 of its terms, far below any change of arithmetic
        assert rel(b["G"], a["G"]) <= 370 * 2.0 ** -24
    co, _ = ec.forward(L.MODE_STREAM_ATTN)                      # and a differing bit is no mismatch there: neither pass streams
    out = {"dpatches": torch.zeros_like(a["dpatches"]), "dtext": torch.zeros_like(a["dtext"]), "G": torch.zeros_like(a["G"])}
    check(ec.backward_rc(0, co, out), "encoder_backward")
    torch.cuda.synchronize()


def test_backward_with_another_bit_than_its_forward_is_refused():
    ec = EncoderCase(240)
    d = ec.d
    for fwd, bwd in ((L.MODE_STREAM_ATTN, 0), (0, L.MODE_STREAM_ATTN)):
        # fresh sentinel-filled outputs for each direction: the matching backward at the end of the loop body writes them
        out = {"dpatches": torch.full((d.B * d.P, d.patch_k), 7.0, dtype=torch.bfloat16, device=DEV),
               "dtext": torch.full((d.B * d.L, d.D), 7.0, device=DEV), "G": torch.full((int(ec.lay.total),), 7.0, device=DEV)}
        co, _ = ec.forward(fwd)
        assert ec.backward_rc(bwd, co, out) == -1 and b"RMCL_MODE_STREAM_ATTN" in lib.rmcl_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in out.values())                      # refused before anything is written
        check(ec.backward_rc(fwd, co, out), "encoder_backward")                       # the matching bit is accepted on the same stash
        torch.cuda.synchronize()
        assert not bool((out["dtext"] == 7.0).all())


# ---- engine against the fp32 engine ---------------------------------------------------------------------------------------------
def compare_step(tol, loss_lp, loss_32, m_lp, m_32, what):
    print(f"{what}: loss bf16 long_sequences {float(loss_lp):.6f}  fp32 {float(loss_32):.6f}")
    assert abs(float(loss_lp) - float(loss_32)) < tol["loss"] * abs(float(loss_32)), what
    p32 = dict(m_32.named_parameters())
    worst = (0.0, None)
    n_checked = 0
    for n, t in m_lp.named_parameters():
        g32 = p32[n].grad
        assert (t.grad is None) == (g32 is None), n
        if g32 is None:
            continue
        a, b = float(t.grad.double().norm()), float(g32.double().norm())
        assert abs(a - b) <= tol["grad"] * b + 2e-7, (what, n, a, b)
        worst = max(worst, (abs(a - b) / max(b, 1e-30), n)) if b > 1e-6 else worst
        n_checked += 1
    assert n_checked > 30
    print(f"{what}: {n_checked} gradients, worst norm difference {worst[0]:.3e} ({worst[1]})")
    # direction, not only length: the element-wise rule those tests apply to slices of the pooler, first qkv and head weight gradients
    # (atol = grad * 2.5 * max |reference|), here on the whole tensors; the same figure is printed for every other parameter
    ratios = {}
    for n, t in m_lp.named_parameters():
        if t.grad is not None and float(p32[n].grad.abs().max()) > 0:
            ratios[n] = float((t.grad.double() - p32[n].grad.double()).abs().max() / p32[n].grad.double().abs().max())
    held = [n for n in ratios if n in ("pooler.dense.weight", "transformer.blocks.0.attn.qkv.weight") or
            (n.endswith(".weight") and n.startswith(("vqa_classifier", "nlvr2_classifier", "rank_output")))]
    top = sorted(ratios.items(), key=lambda kv: -kv[1])[:3]
    print(f"{what}: max |a - b| / max |b| held on {len(held)} tensors, worst {max(ratios[n] for n in held):.3e}; "
          f"over all parameters: " + ", ".join(f"{k} {v:.3e}" for k, v in top))
    assert len(held) >= 3
    for n in held:
        assert float((dict(m_lp.named_parameters())[n].grad - p32[n].grad).abs().max()) <= tol["grad"] * 2.5 * float(p32[n].grad.abs().max()) + 2e-7, (what, n, ratios[n])


def logits_close(tol, got, ref, what):
    """tests/test_vqa_gpu.py / test_nlvr2_gpu.py: atol = logits * max(1, max |reference|)"""
    err = float((got.double() - ref.double()).abs().max())
    print(f"{what}: logits max |d| {err:.3e}, max |reference| {float(ref.abs().max()):.3f}")
    assert got.shape == ref.shape and err <= tol["logits"] * max(1.0, float(ref.abs().max())), (what, err)


def wide(batch, seed, keys=("image",), sizes=SIZES):
    """the batch with its image views replaced by a zero-padded [B, 3, 384, 640] batch of images of `sizes` (BaseDataset.collate pads
    bottom / right with zeros); the oracle's synthetic batches are square (image_size x image_size) and cannot hold a 384 x 640 image"""
    g = torch.Generator().manual_seed(seed)
    hm, wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    for i, k in enumerate(keys):
        sz = sizes if i % 2 == 0 else sizes[::-1]
        img = torch.rand(len(sz), 3, hm, wm, generator=g) * 2 - 1
        for b, (h, w) in enumerate(sz):
            img[b, :, h:, :] = 0
            img[b, :, :, w:] = 0
        batch[k] = [img]
    assert tuple(batch[keys[0]][0].shape) == (3, 3, 384, 640)
    return batch


def assert_streamed(m, tokens=281):
    eng = m.engine
    assert eng.long_sequences and eng.token_cap == 512
    assert any(pb.d.L + 1 + pb.d.P == tokens and eng.stream_bit(pb.d) == L.MODE_STREAM_ATTN for pb in eng._bufs.values())


def vqa_case(K=1):
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=3, adv_steps_img=K, vqav2_label_size=V.N_LABELS)
    p = dict(O.init_params(cfg, 15), **V.vqa_init_params(cfg, 16))
    batch = wide(O.synthetic_batch(cfg, 3, 17, ragged_text=True), 19)
    batch["vqa_labels"], batch["vqa_scores"] = V.synthetic_labels(3, 18)
    return cfg, p, batch


def test_vqa_step_at_281_tokens():
    cfg, p, batch = vqa_case()
    with pytest.raises(NotImplementedError, match="256-token limit"):                     # the default config still refuses
        vqa_step(make_vqa_module(cfg, p, "bf16"), dev_batch(batch))
    m_lp, m_32 = make_vqa_module(cfg, p, "bf16", long_sequences=True), make_vqa_module(cfg, p, "f32")
    compare_step(TOL_VQA["bf16"], vqa_step(m_lp, dev_batch(batch)), vqa_step(m_32, dev_batch(batch)), m_lp, m_32, "vqa")
    logits_close(TOL_VQA["bf16"], m_lp.engine.vqa_bufs(3, "vqa").logits, m_32.engine.vqa_bufs(3, "vqa").logits, "vqa")
    assert_streamed(m_lp)


def test_nlvr2_pair_step_at_281_tokens():
    cfg = O.default_config(num_layers=2, num_negative=1024, adv_steps_img=1, per_gpu_batchsize=3)
    p = O.init_params(cfg, 25)
    p.update(N.nlvr2_init_params(cfg, p, 26))
    batch = wide(N.synthetic_pairs(cfg, 3, 27, ragged_text=True), 28, keys=("image_0", "image_1"))   # image_1: the sizes in reverse order
    m_lp, m_32 = make_nlvr2_module(cfg, p, "bf16", long_sequences=True), make_nlvr2_module(cfg, p, "f32")
    r_lp, r_32 = run_nlvr2(m_lp, dev_batch(batch)), run_nlvr2(m_32, dev_batch(batch))
    compare_step(TOL_NLVR2["bf16"], r_lp["nlvr2_loss"], r_32["nlvr2_loss"], m_lp, m_32, "nlvr2")
    logits_close(TOL_NLVR2["bf16"], r_lp["nlvr2_logits"], r_32["nlvr2_logits"], "nlvr2")
    assert_streamed(m_lp)


def test_itm_irtr_step_at_281_tokens():
    """loss_names itm = 1, irtr = 1 (as tests/test_irtr_gpu.py test_two_steps_move_row_1_with_rank_output_and_leave_row_0 builds it): the ITM
    pass with its word-patch alignment (the IPOT kernel at 240 image tokens) and the ranking pass over B * 3 sequences, both at 281 tokens;
    the 50 / 50 draw of the ITM labels is fixed to the same labels on both engines."""
    cfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=3)
    cfg["draw_false_text"] = 2
    p = O.init_params(cfg, 35)
    batch = wide(R.irtr_batch(cfg, 3, 2, 36), 37, keys=("image", "false_image_0"))
    over = dict(max_image_len=-1, loss_names=_loss_names({"itm": 1, "irtr": 1}))

    def step(dtype, **kw):
        m = make_irtr_module(cfg, p, dtype, **over, **kw)
        m.itm_labels_override = torch.tensor([1, 0, 1])
        r = run_irtr(m, dev_batch(batch))
        assert m.current_tasks == ["itm", "irtr"]
        return m, r, sum(v for k, v in r.items() if "loss" in k)
    with pytest.raises(NotImplementedError, match="256-token limit"):                     # the default config still refuses
        step("bf16")
    (m_lp, r_lp, loss_lp), (m_32, r_32, loss_32) = step("bf16", long_sequences=True), step("f32")
    print("itm + irtr losses:", {k: (float(r_lp[k]), float(r_32[k])) for k in r_32 if "loss" in k})
    compare_step(TOL_IRTR["bf16"], loss_lp, loss_32, m_lp, m_32, "itm + irtr")
    s32 = r_32["irtr_scores"]
    assert float((r_lp["irtr_scores"] - s32).abs().max()) <= TOL_IRTR["bf16"]["logits"] * max(1.0, float(s32.abs().max()))
    assert_streamed(m_lp)


def test_attacked_vqa_step_at_281_tokens():
    cfg, p, batch = vqa_case(K=2)
    first = {}

    def step(dtype, **over):
        m = make_vqa_module(cfg, p, dtype, attacked=True, **over)
        eng, orig = m.engine, m.engine.encoder_backward

        def spy(pb, mode, patchesT, dxn, cls_only, dpatches, dtext=None):
            orig(pb, mode, patchesT, dxn, cls_only, dpatches, dtext)
            if dpatches is not None and dtype not in first:
                first[dtype] = dpatches.float().clone()                                   # the patch gradient of the first PGD step
        eng.encoder_backward = spy
        return m, vqa_step(m, dev_batch(batch))
    m_lp, loss_lp = step("bf16", long_sequences=True)
    m_32, loss_32 = step("f32")
    compare_step(TOL_VQA["bf16"], loss_lp, loss_32, m_lp, m_32, "vqa_attacked")
    a, b = float(first["bf16"].double().norm()), float(first["f32"].double().norm())
    print(f"first PGD step patch gradient: norm bf16 {a:.6e} fp32 {b:.6e}, |a - b| / |b| of the tensor {rel(first['bf16'], first['f32']):.3e}")
    assert first["bf16"].shape == first["f32"].shape and b > 0 and abs(a - b) <= TOL_VQA["bf16"]["grad"] * b + 2e-7
    assert float((first["bf16"] - first["f32"]).abs().max()) <= TOL_VQA["bf16"]["grad"] * 2.5 * float(first["f32"].abs().max())   # element-wise, as above
    logits_close(TOL_VQA["bf16"], m_lp.engine.vqa_bufs(3, "vqa_att").logits, m_32.engine.vqa_bufs(3, "vqa_att").logits, "vqa_attacked")
    assert_streamed(m_lp)


# ---- recall and refusals ----------------------------------------------------------------------------------------------------------
def recall_scenario(width6=576):
    cfg, p, _ = R.case_inputs("irtr_L2_B2_F3")
    gen = torch.Generator().manual_seed(3)
    ids, masks, _ = R.synthetic_text(cfg, 10, 9)
    text_dset = [{"text_ids": ids, "text_masks": masks, "img_index": list(range(10))}]
    image_dset = [{"image": [torch.rand(1, 3, 384, width6 if i == 6 else 384, generator=gen) * 2 - 1], "img_index": [i]} for i in range(10)]
    return cfg, p, text_dset, image_dset


def test_recall_with_an_image_of_257_tokens():
    cfg, p, text_dset, image_dset = recall_scenario()
    m = make_irtr_module(cfg, p, "bf16", max_image_len=-1)
    m.eval()
    with pytest.raises(NotImplementedError, match=r"max_image_len <= 215.*f32.*long_sequences"):   # default config: refused, third way out named last
        objectives.compute_irtr_recall(m, text_dset, image_dset)
    m_lp = make_irtr_module(cfg, p, "bf16", max_image_len=-1, long_sequences=True)
    m_lp.eval()
    got = objectives.compute_irtr_recall(m_lp, text_dset, image_dset, return_scores=True)[6]
    assert got.shape == (10, 10) and torch.isfinite(got).all()
    m_32 = make_irtr_module(cfg, p, "f32", max_image_len=-1)
    m_32.eval()
    ref = objectives.compute_irtr_recall(m_32, text_dset, image_dset, return_scores=True)[6]
    err = float((got.cpu() - ref.cpu()).abs().max())
    print("recall at 257 tokens: max score difference bf16 long_sequences vs fp32", err, "max |score|", float(ref.abs().max()))
    assert err <= TOL_IRTR["bf16"]["logits"] * max(1.0, float(ref.abs().max()))
    rp = m_lp.engine._rank_pass
    assert rp is not None and m_lp.engine.stream_bit(rp.d) == L.MODE_STREAM_ATTN


def test_513_tokens_are_refused_under_long_sequences():
    cfg, p, text_dset, image_dset = recall_scenario(width6=1280)                        # 12 x 40 = 480 patches + 1 + 40 = 521 tokens
    m = make_irtr_module(cfg, p, "bf16", max_image_len=-1, long_sequences=True)
    m.eval()
    calls, orig = [], m.engine.visual_embed
    m.engine.visual_embed = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    with pytest.raises(NotImplementedError, match=r"512-token limit.*max_image_len <= 471"):
        objectives.compute_irtr_recall(m, text_dset, image_dset)
    # the over-long image is counted, not embedded, and the loop goes on to the last image: with several ranks every one of them
    # reaches the reduction of the longest image and raises there, none stops early
    assert len(calls) == 9 and m.engine._rank_pass is None
    m.engine.visual_embed = orig
    eng = m.engine
    with pytest.raises(NotImplementedError, match="512-token limit"):                     # 472 patches: 513 tokens exactly
        eng.rank_forward(text_dset[0]["text_ids"][:1], text_dset[0]["text_masks"][:1], torch.zeros(1, 473, 768, device=DEV),
                         torch.ones(1, 473, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), 472)
    img = torch.rand(2, 3, 384, 1280) * 2 - 1
    with pytest.raises(NotImplementedError, match="512-token limit"):
        eng.bind_batch(text_dset[0]["text_ids"][:2].to(DEV), text_dset[0]["text_masks"][:2].to(DEV), img.to(DEV), tag="irtr")
    # an fp32 engine ignores the key: no limit, no mode bit
    m32 = make_irtr_module(cfg, p, "f32", max_image_len=-1, long_sequences=True)
    assert not m32.engine.long_sequences and m32.engine.stream_bit(L.Dims(L=40, P=300)) == 0
