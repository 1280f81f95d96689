"""-m gpu: VQAv2 fine-tuning (vqa / vqa_attacked) - the HIP head / BCE kernels against torch in fp64, the whole clean and
PGD-attacked steps against the reference's own run (tests/golden/vqa_*.npz from tools/gen_golden_vqa.py) and against the CPU oracle
(tests/vqa_oracle.py), plus the module-level contracts: checkpoint order, optimizer groups, config errors, no PGD weight gradients."""
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P  # noqa: E402
from rmcl_amd.runtime import vqa_layout, stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_finetune_vqa, task_finetune_vqa_randaug_attacked, task_moco  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402
from tests.golden_util import digest  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"
C = L.C
F = C.c_float
HEAD = ("vqa_classifier.0.weight", "vqa_classifier.0.bias", "vqa_classifier.1.weight", "vqa_classifier.1.bias",
        "vqa_classifier.3.weight", "vqa_classifier.3.bias")


# ---- kernels ------------------------------------------------------------------------------------------------------------
def _kernel_case(B, seed, hidden=768):
    cfg = {"hidden_size": hidden, "vqav2_label_size": V.N_LABELS}
    h, specs, n = vqa_layout(cfg, 0)
    g = torch.Generator().manual_seed(seed)
    arena = torch.zeros(n)
    w = {}
    for name, off, shape in specs:
        if name.endswith("1.weight"):
            t = 1 + 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 2:
            t = torch.randn(shape, generator=g) / shape[1] ** 0.5 * (4.0 if name.endswith("3.weight") else 1.0)
        else:
            t = 0.3 * torch.randn(shape, generator=g) - (1.0 if name.endswith("3.bias") else 0.0)
        arena[off:off + t.numel()] = t.flatten()
        w[name] = t.double().requires_grad_(True)
    cls = torch.randn(B, hidden, generator=g)
    # label tables: row 0 empty, row 1 a duplicate label, rows with up to 10 answers, -1 pads; the widest row sets A
    labels, scores = [], []
    for b in range(B):
        k = 0 if b == 0 else (10 if b % 3 == 2 else 1 + b % 4)
        ls = torch.randint(0, V.N_LABELS, (k,), generator=g).tolist()
        if b == 1 and k >= 2:
            ls[-1] = ls[0]
        labels.append(ls)
        scores.append(torch.rand(k, generator=g).tolist())
    A = max(1, max(len(r) for r in labels))
    lab = torch.full((B, A), -1, dtype=torch.int32)
    sco = torch.zeros(B, A)
    for b, (ls, ss) in enumerate(zip(labels, scores)):
        lab[b, :len(ls)] = torch.tensor(ls, dtype=torch.int32)
        sco[b, :len(ss)] = torch.tensor(ss)
    return h, specs, arena.to(DEV), w, cls, labels, scores, lab.to(DEV), sco.to(DEV), A


def _run_kernels(h, arena, cls, lab, sco, A, B, grads, gscale=1.0):
    stash = torch.empty(int(lib.rmcl_vqa_stash_floats(C.byref(h), B)), device=DEV)
    logits = torch.full((B, h.ldl), float("nan"), device=DEV)
    dz = torch.full((B, h.ldl), float("nan"), device=DEV)
    rows = torch.empty(B, 2, device=DEV)
    am = torch.empty(B, dtype=torch.int32, device=DEV)
    loss2 = torch.empty(2, device=DEV)
    dcls = torch.empty(B, h.D, device=DEV)
    gs = torch.tensor([gscale], device=DEV)
    check(lib.rmcl_vqa_head_forward(C.byref(h), P(arena), P(cls), B, P(stash), P(logits), stream_ptr()))
    check(lib.rmcl_vqa_bce(P(logits), h.ldl, P(lab), P(sco), A, B, h.N, F(1.0), P(gs), P(dz), P(rows), P(am), P(loss2), stream_ptr()))
    check(lib.rmcl_vqa_head_backward(C.byref(h), P(arena), P(stash), P(dz), B, P(grads), P(dcls), stream_ptr()))
    torch.cuda.synchronize()
    return logits, dz, rows, am, loss2, dcls


# hidden 256 is H = 512: the narrowest LayerNorm row pass the launcher takes (two float4 per lane; hidden 768 has six)
@pytest.mark.parametrize("B,hidden", [pytest.param(1, 768, id="1"), pytest.param(7, 768, id="7"), pytest.param(64, 768, id="64"),
                                      pytest.param(256, 768, id="256"), pytest.param(1, 256, id="1-h256"), pytest.param(7, 256, id="7-h256")])
def test_vqa_head_and_bce_match_torch_fp64(B, hidden):
    h, specs, arena, w, cls, labels, scores, lab, sco, A = _kernel_case(B, 100 + B + (0 if hidden == 768 else hidden), hidden)
    grads = torch.zeros_like(arena)
    logits, dz, rows, am, loss2, dcls = _run_kernels(h, arena, cls.to(DEV), lab, sco, A, B, grads, gscale=0.5)
    N = h.N
    xd = cls.double().requires_grad_(True)
    zt = V.vqa_head(w, xd)
    tgt = V.dense_targets(labels, scores, B, dtype=torch.float64)
    loss = V.vqa_loss(zt, tgt)
    (0.5 * loss).backward()
    z = logits[:, :N].cpu().double()
    assert float((z - zt.detach()).abs().max()) < 1e-4 * max(1.0, float(zt.abs().max()))
    assert abs(float(loss2[0]) - float(loss)) < 1e-5 * float(loss)
    # dz: 0.5 (sigmoid(z) - t) / B; pad columns exactly 0
    dzt = 0.5 * (torch.sigmoid(zt.detach()) - tgt) / B
    assert float((dz[:, :N].cpu().double() - dzt).abs().max()) < 1e-6
    assert torch.count_nonzero(dz[:, N:]) == 0
    # argmax: the first maximum (NaN pads of the logits buffer never win); score = t[argmax]
    amc = am.cpu().long()
    assert bool((amc < N).all())
    top2 = zt.detach().topk(2, dim=1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 1e-4
    assert torch.equal(amc[clear], zt.detach().argmax(1)[clear])
    sc = tgt.gather(1, amc.view(-1, 1)).squeeze(1)
    assert torch.allclose(rows[:, 1].cpu().double(), sc, atol=1e-7)
    assert abs(float(loss2[1]) - float(sc.mean())) < 1e-6
    # per-row BCE sums
    rb = torch.nn.functional.binary_cross_entropy_with_logits(zt.detach(), tgt, reduction="none").sum(1)
    assert torch.allclose(rows[:, 0].cpu().double(), rb, rtol=1e-5)
    # dense targets (the returned vqa_targets)
    dense = torch.empty(B, N, device=DEV)
    check(lib.rmcl_vqa_targets_dense(P(lab), P(sco), A, B, N, P(dense), N, stream_ptr()))
    assert torch.equal(dense.cpu(), tgt.float())
    # data and parameter gradients
    assert float((dcls.cpu().double() - xd.grad).abs().max()) < 2e-4 * float(xd.grad.abs().max())
    for name, off, shape in specs:
        got = grads[off:off + w[name].numel()].view(shape).cpu().double()
        ref = w[name].grad
        assert float((got - ref).abs().max()) < 2e-4 * float(ref.abs().max()) + 1e-9, name
    w3 = dict((n_, o) for n_, o, _ in specs)["vqa_classifier.3.weight"]
    assert torch.count_nonzero(grads[w3 + N * h.H: w3 + h.ldl * h.H]) == 0           # the pad rows of W3 get no gradient


def test_vqa_kernels_are_bit_reproducible_and_pgd_mode_writes_no_gradient():
    B = 64
    h, specs, arena, w, cls, labels, scores, lab, sco, A = _kernel_case(B, 7)
    c = cls.to(DEV)
    g1, g2 = torch.zeros_like(arena), torch.zeros_like(arena)
    r1 = _run_kernels(h, arena, c, lab, sco, A, B, g1)
    r2 = _run_kernels(h, arena, c, lab, sco, A, B, g2)
    assert torch.equal(r1[0][:, :h.N], r2[0][:, :h.N])                         # logits (the pad columns are not written)
    for a, b in zip(r1[1:], r2[1:]):                                             # dz, rows, argmax, loss2, dcls
        assert torch.equal(a, b)
    assert torch.equal(g1, g2)
    # data-gradient-only backward (the PGD loop): same dcls, no write into the gradient arena
    stash = torch.empty(int(lib.rmcl_vqa_stash_floats(C.byref(h), B)), device=DEV)
    logits = torch.empty(B, h.ldl, device=DEV)
    check(lib.rmcl_vqa_head_forward(C.byref(h), P(arena), P(c), B, P(stash), P(logits), stream_ptr()))
    dcls = torch.empty(B, 768, device=DEV)
    check(lib.rmcl_vqa_head_backward(C.byref(h), P(arena), P(stash), P(r1[1]), B, None, P(dcls), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dcls, r1[5])


# ---- module -------------------------------------------------------------------------------------------------------------
def make_vqa_module(ocfg, p, dtype="f32", attacked=False, **over):
    kw = dict(num_layers=ocfg["num_layers"], per_gpu_batchsize=ocfg["per_gpu_batchsize"], adv_steps_img=ocfg["adv_steps_img"],
              drop_rate=0.0, max_steps=100, warmup_steps=0)
    kw.update(over)
    cfg = task_finetune_vqa_randaug_attacked(image_view=True, **kw) if attacked else task_finetune_vqa(**kw)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype=dtype)
    sd = {n: t.to(DEV) for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    m.train()
    return m


def _step(m, batch):
    m.zero_grad()
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    return loss


# fp32 engine: the repository's fp32 contract (1e-3 on the loss); bf16 engine: the bf16 class of the golden tests (8-bit mantissa
# operands in the encoder GEMMs, fp32 accumulation and fp32 head)
TOL = {"f32": dict(loss=1e-3, logits=2e-3, grad=2e-3, delta=5e-5), "bf16": dict(loss=1e-2, logits=0.1, grad=0.1, delta=2e-3)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", V.FIXTURES)
def test_vqa_step_matches_reference_golden(name, dtype):
    g, cfg, p, batch, targets, attacked = V.load_case(name)
    tol = TOL[dtype]
    m = make_vqa_module(cfg, p, dtype, attacked)
    db = dev_batch(batch)
    loss = _step(m, db)
    task = "vqa_attacked" if attacked else "vqa"
    assert abs(float(loss) - float(g["vqa_loss"])) < tol["loss"] * float(g["vqa_loss"])
    assert abs(float(m.logged[f"{task}/train/loss"]) - float(g[f"log_{task}__train__loss"])) < tol["loss"] * float(g["vqa_loss"])
    assert abs(float(m.logged[f"{task}/train/score"]) - float(g[f"log_{task}__train__score"])) < 1e-6
    B = cfg["per_gpu_batchsize"]
    eng = m.engine
    vb = eng.vqa_bufs(B, "vqa_att" if attacked else "vqa")
    lg = vb.logits.cpu().numpy()
    np.testing.assert_allclose(lg, g["vqa_logits"], atol=tol["logits"] * max(1.0, float(np.abs(g["vqa_logits"]).max())))
    if attacked:
        pb = eng.bufs(B, "vqa_att")
        delta = eng.patches_to_image(pb.delta, pb).cpu()
        np.testing.assert_allclose(delta[:, :, ::8, ::8].numpy(), g["delta_sub"], atol=tol["delta"])
        assert abs(float(m.logged["vqa_attacked_attack/train/delta"]) - float(g["log_vqa_attacked_attack__train__delta"])) < \
            (1e-5 if dtype == "f32" else 1e-4)
    params = dict(m.named_parameters())
    for n, d in zip(g["grad_names"], g["grad_digest"]):
        got = digest(params[str(n)].grad)
        assert abs(got[1] - d[1]) <= tol["grad"] * d[1] + 1e-7, (str(n), got[:3], d[:3])
    for key, pname in (("grad_vqa_w0", HEAD[0]), ("grad_vqa_w3", HEAD[4]), ("grad_pooler_w", "pooler.dense.weight")):
        ref = g[key]
        np.testing.assert_allclose(params[pname].grad[:8, :64].cpu().numpy(), ref, atol=tol["grad"] * 2.5 * np.abs(ref).max(), err_msg=key)
    for key, pname in (("grad_vqa_b0", HEAD[1]), ("grad_vqa_g1", HEAD[2]), ("grad_vqa_b1", HEAD[3]), ("grad_vqa_b3", HEAD[5])):
        ref = g[key]
        np.testing.assert_allclose(params[pname].grad[:64].cpu().numpy(), ref, atol=tol["grad"] * 2.5 * np.abs(ref).max(), err_msg=key)
    # the returned dict: reference keys, dense targets, [B, 3129] logits
    with torch.no_grad():
        m.eval()
        out = m(db)
    assert out["vqa_logits"].shape == (B, V.N_LABELS)
    assert torch.equal(out["vqa_targets"].cpu(), targets)
    assert out["vqa_labels"] is db["vqa_labels"] and out["vqa_scores"] is db["vqa_scores"]


def test_vqa_bs64_bf16_matches_oracle():
    """The benchmarked shape (12 layers, bs = 64, bf16 encoder kernels) against the CPU oracle with the same weights and batch."""
    cfg = O.default_config(num_layers=12, per_gpu_batchsize=64, adv_steps_img=1, vqav2_label_size=V.N_LABELS)
    p = dict(O.init_params(cfg, 5), **V.vqa_init_params(cfg, 6))
    batch = O.synthetic_batch(cfg, 64, 7, ragged_text=True)
    labels, scores = V.synthetic_labels(64, 8)
    batch["vqa_labels"], batch["vqa_scores"] = labels, scores
    m = make_vqa_module(cfg, p, "bf16")
    loss = _step(m, dev_batch(batch))
    targets = V.dense_targets(labels, scores, 64)
    torch.set_num_threads(16)
    with torch.no_grad():
        r = V.compute_vqa(p, cfg, batch, targets)
    assert abs(float(loss) - float(r["vqa_loss"])) < 1e-2 * float(r["vqa_loss"])
    lg = m.engine.vqa_bufs(64, "vqa").logits.cpu()
    assert float((lg - r["vqa_logits"]).abs().max()) < 0.1 * max(1.0, float(r["vqa_logits"].abs().max()))
    params = dict(m.named_parameters())
    for n in HEAD:
        assert torch.isfinite(params[n].grad).all() and float(params[n].grad.abs().max()) > 0, n


def test_pgd_loop_leaves_the_gradient_arena_unchanged():
    g, cfg, p, batch, targets, attacked = V.load_case("vqa_att_K2_L2_B4_ragged")
    m = make_vqa_module(cfg, p, "f32", attacked=True)
    eng = m.engine
    eng.g32.fill_(0.25)
    before = eng.g32.clone()
    db = dev_batch(batch)
    delta = m.pgd_attacker.pgd_attack(m, dict(db, image=[db["image"][0]]))
    torch.cuda.synchronize()
    assert float(delta.abs().max()) > 0
    assert torch.equal(eng.g32, before)


def test_checkpoint_order():
    """vilt_module.py:134-164: with test_only=False the checkpoint is applied BEFORE the head exists (its vqa_classifier.* stay at
    init and are reported unused); with test_only=True (:254-268) they are loaded."""
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=2, adv_steps_img=1, vqav2_label_size=V.N_LABELS)
    p = dict(O.init_params(cfg, 1), **V.vqa_init_params(cfg, 2))
    sd = {n: t for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vqa.ckpt")
        torch.save({"state_dict": sd}, path)
        kw = dict(num_layers=2, per_gpu_batchsize=2, drop_rate=0.0, load_path=path)
        torch.manual_seed(0)
        m = ViLTransformerSS(task_finetune_vqa(**kw), device=DEV, compute_dtype="f32")
        msd = m.state_dict()
        assert torch.equal(msd["transformer.blocks.1.attn.qkv.weight"].cpu(), sd["transformer.blocks.1.attn.qkv.weight"])
        for n in HEAD:
            assert n in m.load_report["unexpected"], n
            assert not torch.equal(msd[n].cpu(), sd[n]), n
        assert torch.equal(msd["vqa_classifier.1.weight"].cpu(), torch.ones(2 * 768))      # LayerNorm init (1 / 0), not N(0, 0.02)
        assert torch.equal(msd["vqa_classifier.1.bias"].cpu(), torch.zeros(2 * 768))
        assert torch.equal(msd["vqa_classifier.3.bias"].cpu(), torch.zeros(V.N_LABELS))
        assert abs(float(msd["vqa_classifier.3.weight"].std()) - 0.02) < 1e-3
        m2 = ViLTransformerSS(task_finetune_vqa(test_only=True, **kw), device=DEV, compute_dtype="f32")
        msd2 = m2.state_dict()
        for n in HEAD:
            assert torch.equal(msd2[n].cpu(), sd[n]), n
            assert n not in m2.load_report["unexpected"]


def test_optimizer_groups_of_the_head():
    m = ViLTransformerSS(task_finetune_vqa(num_layers=2, per_gpu_batchsize=2, max_steps=10, weight_decay=0.01), device=DEV, compute_dtype="f32")
    (opt,), _ = m.configure_optimizers()
    ends = opt.seg_end.cpu().tolist()
    for name, off, shape in m.engine.specs:
        if not name.startswith("vqa_classifier"):
            continue
        i = next(j for j, e in enumerate(ends) if e > off)
        decay, head = O.param_group(name)
        assert float(opt.seg_wd[i]) == pytest.approx(0.01 if decay else 0.0), name
        assert float(opt.seg_mult[i]) == pytest.approx(10.0 if head else 1.0), name
    decay, head = O.param_group("vqa_classifier.1.weight")
    assert decay and head                                # the head's LayerNorm gain is decayed, at lr x lr_mult (vilt_utils.py:335-393)


def test_config_errors():
    kw = dict(num_layers=2, per_gpu_batchsize=2)
    with pytest.raises(ValueError):
        ViLTransformerSS(task_finetune_vqa_randaug_attacked(**kw), device=DEV, compute_dtype="f32")       # both views off
    with pytest.raises(NotImplementedError):
        ViLTransformerSS(task_finetune_vqa_randaug_attacked(text_view=True, **kw), device=DEV, compute_dtype="f32")
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=2)
    m = ViLTransformerSS(task_finetune_vqa(drop_rate=0.0, **kw), device=DEV, compute_dtype="f32")
    batch = dev_batch(O.synthetic_batch(cfg, 2, 3))
    batch["vqa_labels"], batch["vqa_scores"] = [[1], [V.N_LABELS]], [[1.0], [1.0]]
    with pytest.raises(ValueError):
        m.training_step(batch, 0)


def test_test_step_returns_qids_and_answers():
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=3, vqav2_label_size=V.N_LABELS)
    m = ViLTransformerSS(task_finetune_vqa(num_layers=2, per_gpu_batchsize=3, drop_rate=0.0), device=DEV, compute_dtype="f32")
    batch = dev_batch(O.synthetic_batch(cfg, 3, 4))
    batch["vqa_labels"], batch["vqa_scores"] = [[], [5], [7, 7]], [[], [1.0], [0.3, 0.6]]
    batch["qid"] = [11, 12, 13]
    out = m.test_step(batch, 0)
    assert out["qids"] == [11, 12, 13] and all(isinstance(x, int) for x in out["preds"])
    m.id2answer = {i: f"a{i}" for i in range(V.N_LABELS)}
    out2 = m.test_step(batch, 0)
    assert out2["preds"] == [f"a{i}" for i in out["preds"]]


def test_adamw_loop_with_dropout_lowers_the_loss():
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=8, vqav2_label_size=V.N_LABELS)
    m = ViLTransformerSS(task_finetune_vqa(num_layers=2, per_gpu_batchsize=8, drop_rate=0.1, max_steps=100, warmup_steps=0),
                         device=DEV, compute_dtype="bf16")
    (opt,), _ = m.configure_optimizers()
    batch = O.synthetic_batch(cfg, 8, 5, ragged_text=True)
    batch["vqa_labels"], batch["vqa_scores"] = V.synthetic_labels(8, 6)
    batch = dev_batch(batch)
    m.train()
    losses = []
    for it in range(20):
        m.zero_grad()
        loss = m.training_step(batch, it)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses


def test_moco_model_is_unchanged_by_the_vqa_head():
    cfg = task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=2, image_view=True)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype="f32")
    eng = m.engine
    assert eng.vqa is None and not eng.vqa_specs
    assert eng.total == int(eng.layout.total) and eng.q32.numel() == eng.g32.numel() == int(eng.layout.total)
    assert not any("vqa" in k for k in m.state_dict())
