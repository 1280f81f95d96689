"""-m gpu: NLVR2 fine-tuning (nlvr2 / nlvr2_attacked) - the cross-entropy kernel against torch in fp64, the image token-type kernels
(row 2, per-pair rows, where their gradients land), the pair pass against the two-pass form, the clean and PGD-attacked steps against
the reference's own run (tests/golden/nlvr2_*.npz from tools/gen_golden_nlvr2.py) and against the CPU oracle (tests/nlvr2_oracle.py),
plus the module contracts: checkpoint rules, optimizer groups, config errors, no PGD weight gradients, validation logs."""
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
from rmcl_amd.runtime import stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_finetune_nlvr2, task_finetune_nlvr2_randaug_attacked, task_moco  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, vilt_utils  # noqa: E402
from tests import nlvr2_oracle as N  # noqa: E402
from tests.golden_util import digest  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"
C = L.C
F = C.c_float
HEAD = ("nlvr2_classifier.0.weight", "nlvr2_classifier.0.bias", "nlvr2_classifier.1.weight", "nlvr2_classifier.1.bias",
        "nlvr2_classifier.3.weight", "nlvr2_classifier.3.bias")
TT = "token_type_embeddings.weight"


# ---- cross-entropy kernel -------------------------------------------------------------------------------------------------
def _ce(logits_p, ldl, labels, N, gscale=1.0, gdev=None, ref=None):
    B = logits_p.shape[0]
    dz = torch.full((B, ldl), float("nan"), device=DEV)
    rows = torch.empty(B, device=DEV)
    am = torch.empty(B, dtype=torch.int32, device=DEV)
    stats = torch.empty(3, device=DEV)
    check(lib.rmcl_nlvr2_ce(P(logits_p), ldl, P(labels), B, N, F(gscale), P(gdev), P(dz), P(rows), P(am), P(ref), ldl, P(stats),
                            stream_ptr()))
    torch.cuda.synchronize()
    return dz, rows, am, stats


@pytest.mark.parametrize("B,N", [(1, 2), (5, 2), (64, 2), (300, 2), (33, 7)])
def test_ce_kernel_matches_torch_fp64(B, N):
    g = torch.Generator().manual_seed(B * 31 + N)
    ldl = 64
    z = torch.full((B, ldl), float("nan"))
    z[:, :N] = 3 * torch.randn(B, N, generator=g)
    z[0, :N] = 0.25                                                  # a tie: the first maximum wins
    ref = torch.full((B, ldl), float("nan"))
    ref[:, :N] = 3 * torch.randn(B, N, generator=g)
    lab = torch.randint(0, N, (B,), generator=g)
    zd, refd, labd = z.to(DEV), ref.to(DEV), lab.to(torch.int32).to(DEV)
    dz, rows, am, stats = _ce(zd, ldl, labd, N, 0.5, torch.tensor([0.25], device=DEV), refd)
    zt = z[:, :N].double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(zt, lab)
    (0.125 * loss).backward()
    assert abs(float(stats[0]) - float(loss)) < 1e-6 * max(1.0, float(loss))
    assert torch.allclose(rows.cpu().double(), torch.nn.functional.cross_entropy(zt.detach(), lab, reduction="none"), atol=2e-6)
    assert float((dz[:, :N].cpu().double() - zt.grad).abs().max()) < 1e-7
    assert torch.count_nonzero(dz[:, N:]) == 0
    amt = z[:, :N].argmax(1)
    assert torch.equal(am.cpu().long(), amt) and int(am[0]) == 0
    assert float(stats[1]) == float((amt == lab).sum())
    assert float(stats[2]) == float((amt != ref[:, :N].argmax(1)).sum())
    dz2, rows2, am2, stats2 = _ce(zd, ldl, labd, N, 0.5, torch.tensor([0.25], device=DEV), refd)
    for a, b in ((dz, dz2), (rows, rows2), (am, am2), (stats, stats2)):   # no float atomics: bit-reproducible
        assert torch.equal(a, b)
    _, _, _, st3 = _ce(zd, ldl, labd, N)                               # no reference logits: no change count
    assert float(st3[2]) == 0.0


# ---- modules ----------------------------------------------------------------------------------------------------------------
def make_module(cfg, p, dtype="f32", attacked=False, **over):
    kw = dict(num_layers=cfg["num_layers"], per_gpu_batchsize=cfg["per_gpu_batchsize"], adv_steps_img=cfg["adv_steps_img"],
              drop_rate=0.0, max_steps=100, warmup_steps=0)
    kw.update(over)
    c = task_finetune_nlvr2_randaug_attacked(image_view=True, **kw) if attacked else task_finetune_nlvr2(**kw)
    m = ViLTransformerSS(c, device=DEV, compute_dtype=dtype)
    sd = {n: t.to(DEV) for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    m.train()
    return m


def _run(m, batch, train=True):
    """forward of the module's tasks; train: also the backward of every loss key (what training_step sums)"""
    vilt_utils.set_task(m)
    m.zero_grad()
    m.train(train)
    if train:
        ret = m(batch)
        total = sum(v for k, v in ret.items() if "loss" in k)
        total.backward()
    else:
        with torch.no_grad():
            ret = m(batch)
    torch.cuda.synchronize()
    return ret


def _small(seed=3, B=4, L=2, sizes=True):
    cfg = O.default_config(num_layers=L, per_gpu_batchsize=B, adv_steps_img=2)
    p = O.init_params(cfg, seed)
    p.update(N.nlvr2_init_params(cfg, p, seed + 1))
    s0 = [(384, 320), (256, 384), (320, 320), (384, 384)][:B] if sizes else None
    s1 = [(320, 384), (384, 256), (288, 352), (352, 224)][:B] if sizes else None
    return cfg, p, N.synthetic_pairs(cfg, B, seed + 2, ragged_text=True, sizes0=s0, sizes1=s1)


def test_image_token_type_2_equals_row_1_holding_row_2():
    cfg, p, batch = _small(sizes=False)
    m = make_module(cfg, p)
    db = dev_batch(batch)
    with torch.no_grad():
        a = m.infer(db, image_token_type_idx=2)["cls_feats"].clone()
        assert not torch.equal(a, m.infer(db, image_token_type_idx=1)["cls_feats"])          # row 2 is not row 1
        tt = dict(m.named_parameters())[TT]
        tt[1].copy_(tt[2])
        m.engine.lp_stale = True
        b = m.infer(dict(db, image_0=db["image_1"]), image_token_type_idx=1)["cls_feats"]
    assert torch.equal(a, b)


def test_full_mode_token_type_gradients_land_in_the_rows_used():
    cfg, p, batch = _small(sizes=False)
    m = make_module(cfg, p)
    db = dev_batch(batch)
    for t, (z, nz) in ((1, (2, 1)), (2, (1, 2))):
        m.zero_grad()
        out = m.infer(db, image_token_type_idx=t)
        out["cls_feats"].sum().backward()
        torch.cuda.synchronize()
        g = dict(m.named_parameters())[TT].grad
        assert torch.count_nonzero(g[z]) == 0 and torch.count_nonzero(g[nz]) > 0 and torch.count_nonzero(g[0]) > 0, t
    # the pair pass: image_0's tokens feed row 1, image_1's row 2
    m.zero_grad()
    ret = _run(m, db)
    g = dict(m.named_parameters())[TT].grad
    assert torch.count_nonzero(g[1]) > 0 and torch.count_nonzero(g[2]) > 0 and not torch.equal(g[1], g[2])
    assert torch.isfinite(ret["nlvr2_loss"])


@pytest.mark.parametrize("attacked", [False, True])
def test_pair_pass_equals_two_pass(attacked):
    cfg, p, batch = _small()
    db = dev_batch(batch)
    res = []
    for pair in (True, False):
        m = make_module(cfg, p, "f32", attacked, nlvr2_pair_pass=pair)
        ret = _run(m, db)
        res.append((ret, {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}, dict(m.logged)))
    (r1, g1, l1), (r2, g2, l2) = res
    for k in r1:
        if k.endswith("_loss"):
            assert abs(float(r1[k]) - float(r2[k])) < 1e-6, k
        elif k.endswith("_logits"):
            assert float((r1[k] - r2[k]).abs().max()) < 1e-6, k
    for n in g1:
        scale = float(g2[n].abs().max()) + 1e-12
        assert float((g1[n] - g2[n]).abs().max()) <= 1e-4 * scale + 1e-9, n                 # fp32 summation order only
    if attacked:
        assert abs(float(l1["nlvr2_attacked_attack/train/delta"]) - float(l2["nlvr2_attacked_attack/train/delta"])) < 1e-7


# fp32 engine: the repository's fp32 contract (the VQA tests' tolerances); bf16 engine: 8-bit mantissa operands in the encoder GEMMs
# with fp32 accumulation and an fp32 head - the VQA bf16 class; the delta bound covers PGD components whose small gradients flip
# their step direction under bf16 (a step is lr = 0.05 against eps = 0.005: a delta entry moves by at most eps per decision)
TOL = {"f32": dict(loss=1e-3, logits=2e-3, grad=2e-3, delta=5e-5), "bf16": dict(loss=1e-2, logits=0.1, grad=0.1, delta=2e-3)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", N.FIXTURES)
def test_step_matches_reference_golden(name, dtype):
    g, cfg, p, batch, idx = N.load_case(name)
    tol = TOL[dtype]
    attacked = idx is not None
    m = make_module(cfg, p, dtype, attacked, **({"attack_idx": list(idx)} if attacked else {}))
    db = dev_batch(batch)
    ret = _run(m, db)
    keys = ("nlvr2_original_loss", "nlvr2_attacked_loss") if attacked else ("nlvr2_loss",)
    for k in keys:
        assert abs(float(ret[k]) - float(g[k])) < tol["loss"] * float(g[k]), (k, float(ret[k]), float(g[k]))
        lk = k.replace("_loss", "_logits")
        ref = g[lk]
        np.testing.assert_allclose(ret[lk].cpu().numpy(), ref, atol=tol["logits"] * max(1.0, float(np.abs(ref).max())), err_msg=lk)
    if not attacked:
        assert abs(float(m.logged["nlvr2/train/loss"]) - float(g["log_nlvr2__train__loss"])) < tol["loss"] * float(g["nlvr2_loss"])
    params = dict(m.named_parameters())
    for n, d in zip(g["grad_names"], g["grad_digest"]):
        got = digest(params[str(n)].grad)
        assert abs(got[1] - d[1]) <= tol["grad"] * d[1] + 1e-7, (str(n), got[:3], d[:3])
    for key, pname, sl in (("grad_nlvr2_w0", HEAD[0], (slice(0, 8), slice(0, 64))), ("grad_nlvr2_w3", HEAD[4], (slice(None), slice(0, 64))),
                           ("grad_pooler_w", "pooler.dense.weight", (slice(0, 8), slice(0, 64))), ("grad_nlvr2_b0", HEAD[1], (slice(0, 64),)),
                           ("grad_nlvr2_g1", HEAD[2], (slice(0, 64),)), ("grad_nlvr2_b3", HEAD[5], (slice(None),)), ("grad_token_type", TT, (slice(None),))):
        ref = g[key]
        np.testing.assert_allclose(params[pname].grad[sl].cpu().numpy(), ref, atol=tol["grad"] * 2.5 * np.abs(ref).max(), err_msg=key)
    if attacked:
        d0, d1 = m.pgd_attacker.pgd_attack(m, dict(db, image_0=[db["image_0"][0]], image_1=[db["image_1"][0]]))
        for k, d in enumerate((d0, d1)):
            if not idx[k]:
                assert torch.count_nonzero(d) == 0                      # not attacked: delta exactly 0
            got, ref = d[:, :, ::8, ::8].cpu().numpy(), g[f"delta{k}_sub"]
            if dtype == "f32":
                np.testing.assert_allclose(got, ref, atol=tol["delta"])
            else:
                # bf16: an entry whose gradient is small against the row's max |g| moves by lr * g / max|g| per step, and bf16 operands shift
                # that ratio: such entries may land anywhere inside the clip range.  Bound: every entry within 2 eps (the clip range), and
                # no more than 0.1 % of them beyond tol["delta"]
                err = np.abs(got - ref)
                assert float(err.max()) <= 2 * cfg["adv_max_norm_img"] + 1e-6
                assert float((err > tol["delta"]).mean()) <= 1e-3, float((err > tol["delta"]).mean())
        # validation phase: the reference's logged values (dev / test rows, change_rate_cross, delta)
        m.logged = {}
        _run(m, db, train=False)
        for k in [k for k in g.files if k.startswith("log_")]:
            name_ = k[4:].replace("__", "/")
            atol = 1e-6 if ("accuracy" in k or "change_rate" in k) else (tol["loss"] * 2 * float(g[k]) if "loss" in k else tol["delta"] * 0.2)
            if "accuracy" in k or "change_rate" in k:
                atol = 1e-6 if dtype == "f32" else 0.5                   # (bf16: a near-tie row may flip)
            assert abs(float(m.logged[name_]) - float(g[k])) <= atol, (name_, float(m.logged[name_]), float(g[k]))


def test_bs64_bf16_matches_oracle():
    """The benchmarked shape (12 layers, 64 pairs, bf16 encoder kernels) against the CPU oracle with the same weights and batch."""
    cfg = O.default_config(num_layers=12, per_gpu_batchsize=64, adv_steps_img=1)
    p = O.init_params(cfg, 5)
    p.update(N.nlvr2_init_params(cfg, p, 6))
    batch = N.synthetic_pairs(cfg, 64, 7, ragged_text=True)
    m = make_module(cfg, p, "bf16")
    ret = _run(m, dev_batch(batch))
    torch.set_num_threads(16)
    with torch.no_grad():
        r = N.compute_nlvr2(p, cfg, batch)
    assert abs(float(ret["nlvr2_loss"]) - float(r["nlvr2_loss"])) < 1e-2 * float(r["nlvr2_loss"])
    assert float((ret["nlvr2_logits"].cpu() - r["nlvr2_logits"]).abs().max()) < 0.1 * max(1.0, float(r["nlvr2_logits"].abs().max()))
    params = dict(m.named_parameters())
    for n in HEAD + (TT,):
        assert torch.isfinite(params[n].grad).all() and float(params[n].grad.abs().max()) > 0, n


def test_pgd_loop_leaves_the_gradient_arena_unchanged():
    g, cfg, p, batch, idx = N.load_case("nlvr2_att_K2_L2_B4")
    m = make_module(cfg, p, "f32", attacked=True)
    eng = m.engine
    eng.g32.fill_(0.25)
    before = eng.g32.clone()
    db = dev_batch(batch)
    d0, d1 = m.pgd_attacker.pgd_attack(m, dict(db, image_0=[db["image_0"][0]], image_1=[db["image_1"][0]]))
    torch.cuda.synchronize()
    assert float(d0.abs().max()) > 0 and float(d1.abs().max()) > 0
    assert torch.equal(eng.g32, before)


def test_checkpoint_rules():
    """vilt_module.py:134-160 + :193-231: a pre-training checkpoint (2-row token types) fills rows 0 / 1 and row 2 becomes a copy of row 1;
    nlvr2_classifier.* of a training-time load are not used; under test_only a 3-row checkpoint (and the head) load as they are."""
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=2, adv_steps_img=1)
    p = O.init_params(cfg, 1)
    hp = N.nlvr2_init_params(cfg, p, 2)
    pre = {n: t for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))}
    fine = dict(pre, **hp)
    with tempfile.TemporaryDirectory() as tmp:
        kw = dict(num_layers=2, per_gpu_batchsize=2, drop_rate=0.0)
        path = os.path.join(tmp, "pre.ckpt")
        torch.save({"state_dict": dict(pre, **{k: v for k, v in hp.items() if k != TT})}, path)
        m = ViLTransformerSS(task_finetune_nlvr2(load_path=path, **kw), device=DEV, compute_dtype="f32")
        sd = m.state_dict()
        tt = sd[TT].cpu()
        assert tt.shape == (3, 768)
        assert torch.equal(tt[0], pre[TT][0]) and torch.equal(tt[1], pre[TT][1]) and torch.equal(tt[2], pre[TT][1])
        assert torch.equal(sd["text_embeddings.token_type_embeddings.weight"].cpu(), pre["text_embeddings.token_type_embeddings.weight"])
        for n in HEAD:
            assert n in m.load_report["unexpected"] and not torch.equal(sd[n].cpu(), hp[n]), n
        assert torch.equal(sd["nlvr2_classifier.1.weight"].cpu(), torch.ones(1536))
        assert abs(float(sd["nlvr2_classifier.0.weight"].std()) - 0.02) < 1e-3
        path3 = os.path.join(tmp, "fine.ckpt")
        torch.save({"state_dict": fine}, path3)
        with pytest.raises(RuntimeError):                               # a 3-row table at training time: a size mismatch, as in the reference
            ViLTransformerSS(task_finetune_nlvr2(load_path=path3, **kw), device=DEV, compute_dtype="f32")
        m2 = ViLTransformerSS(task_finetune_nlvr2(load_path=path3, test_only=True, **kw), device=DEV, compute_dtype="f32")
        sd2 = m2.state_dict()
        assert torch.equal(sd2[TT].cpu(), hp[TT])
        for n in HEAD:
            assert torch.equal(sd2[n].cpu(), hp[n]), n
    m3 = ViLTransformerSS(task_finetune_nlvr2(**kw), device=DEV, compute_dtype="f32")        # no checkpoint: rows [0, 1, 1] of the init
    t3 = m3.state_dict()[TT]
    assert torch.equal(t3[2], t3[1]) and not torch.equal(t3[0], t3[1])


def test_optimizer_groups_of_the_head():
    m = ViLTransformerSS(task_finetune_nlvr2(num_layers=2, per_gpu_batchsize=2, max_steps=10, weight_decay=0.01, lr_mult=10),
                         device=DEV, compute_dtype="f32")
    (opt,), _ = m.configure_optimizers()
    ends = opt.seg_end.cpu().tolist()
    seen = 0
    for name, off, shape in m.engine.specs:
        if not name.startswith("nlvr2_classifier"):
            continue
        i = next(j for j, e in enumerate(ends) if e > off)
        decay, head = O.param_group(name)
        assert head
        assert float(opt.seg_wd[i]) == pytest.approx(0.01 if decay else 0.0), name
        assert float(opt.seg_mult[i]) == pytest.approx(10.0), name
        seen += 1
    assert seen == 6


def test_config_errors():
    kw = dict(num_layers=2, per_gpu_batchsize=2)
    with pytest.raises(ValueError):                                     # (b) no view
        ViLTransformerSS(task_finetune_nlvr2_randaug_attacked(**kw), device=DEV, compute_dtype="f32")
    with pytest.raises(ValueError):                                     # (c) attack_idx [False, False]
        ViLTransformerSS(task_finetune_nlvr2_randaug_attacked(image_view=True, attack_idx=[False, False], **kw), device=DEV, compute_dtype="f32")
    with pytest.raises(NotImplementedError):                            # (d) text view
        ViLTransformerSS(task_finetune_nlvr2_randaug_attacked(text_view=True, **kw), device=DEV, compute_dtype="f32")
    cfg, p, batch = _small(B=2, sizes=False)
    m = make_module(cfg, p)
    db = dev_batch(batch)
    with pytest.raises(ValueError):
        m.training_step(dict(db, answers=[True, 2]), 0)
    mm = ViLTransformerSS(task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=2, image_view=True), device=DEV, compute_dtype="f32")
    with pytest.raises(ValueError):                                     # row 2 exists only in NLVR2 models
        with torch.no_grad():
            mm.infer(dict(db, image=db["image_0"]), image_token_type_idx=2)


def test_validation_logs_split_dev_and_test():
    cfg, p, batch = _small(sizes=False)
    m = make_module(cfg, p)
    db = dev_batch(batch)
    ret = _run(m, db, train=False)
    lab = torch.tensor(batch["answers"]).long()
    with torch.no_grad():
        r = N.compute_nlvr2(p, cfg, batch)
    ce = torch.nn.functional.cross_entropy(r["nlvr2_logits"], lab, reduction="none")
    for split, rows in (("dev", [0, 1]), ("test", [2, 3])):
        assert abs(float(m.logged[f"nlvr2/{split}/loss"]) - float(ce[rows].mean())) < 1e-3
        acc = float((r["nlvr2_logits"][rows].argmax(1) == lab[rows]).float().mean())
        assert float(m.logged[f"nlvr2/{split}/accuracy"]) == pytest.approx(acc)
    assert "nlvr2/train/loss" not in m.logged and torch.equal(ret["nlvr2_labels"].cpu(), lab)


def test_adamw_loop_lowers_the_loss():
    cfg, p, batch = _small(B=8, sizes=False)
    m = ViLTransformerSS(task_finetune_nlvr2(num_layers=2, per_gpu_batchsize=8, drop_rate=0.1, max_steps=100, warmup_steps=0),
                         device=DEV, compute_dtype="bf16")
    (opt,), _ = m.configure_optimizers()
    db = dev_batch(batch)
    m.train()
    losses = []
    for it in range(20):
        m.zero_grad()
        loss = m.training_step(db, it)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses


def test_moco_model_is_unchanged_by_nlvr2():
    cfg = task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=2, image_view=True)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype="f32")
    eng = m.engine
    assert eng.nlvr2 is None and not eng.nlvr2_specs
    assert eng.total == int(eng.layout.total) and eng.layout.cls == eng.layout.vtype + 2 * 768
    assert tuple(m.state_dict()[TT].shape) == (2, 768)
    assert not any("nlvr2" in k for k in m.state_dict())
