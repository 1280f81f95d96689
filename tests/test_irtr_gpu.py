"""-m gpu: image-text retrieval (irtr) - the score / cross-entropy / backward kernels against torch in fp64, the itm + irtr step against
the reference's own run (tests/golden/irtr*.npz from tools/gen_golden_irtr.py) on both engines, the rank_output alias over two optimizer
steps, visual_embed and infer(image_embeds=...) against the fixture and against infer on pixels, the tiling invariance of the cached
rank pass, the recall evaluation end to end, and the module contracts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P, I64  # noqa: E402
from rmcl_amd.runtime import stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_finetune_irtr_coco, task_moco, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, vilt_utils, objectives  # noqa: E402
from tests import irtr_oracle as R  # noqa: E402
from tests.golden_util import digest  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"
F = L.C.c_float
# the repository's tolerance classes (tests/test_nlvr2_gpu.py TOL): fp32 engine / bf16 engine
TOL = {"f32": dict(loss=1e-3, logits=2e-3, grad=2e-3), "bf16": dict(loss=1e-2, logits=0.1, grad=0.1)}


# ---- kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Rr", [(1, 2), (5, 4), (7, 16), (13, 64), (3, 1), (66, 16)])
def test_score_ce_backward_kernels_match_torch_fp64(B, Rr):
    g = torch.Generator().manual_seed(B * 100 + Rr)
    S, D = B * Rr, 768
    cls = torch.randn(S, D, generator=g)
    w = 0.2 * torch.randn(D, generator=g)
    b = torch.randn(1, generator=g)
    cd, wd, bd = cls.to(DEV), w.to(DEV), b.to(DEV)
    gdev = torch.tensor([0.25], device=DEV)

    def run():
        scores = torch.full((S,), float("nan"), device=DEV)
        dscore = torch.full((S,), float("nan"), device=DEV)
        rows = torch.empty(B, device=DEV)
        stats = torch.empty(2, device=DEV)
        check(lib.rmcl_irtr_score(P(cd), I64(D), P(wd), P(bd), S, D, P(scores), None, I64(S), stream_ptr()))
        check(lib.rmcl_irtr_ce(P(scores), B, Rr, F(0.5), P(gdev), P(dscore), P(rows), P(stats), stream_ptr()))
        dcls = torch.full((S, D), float("nan"), device=DEV)
        dw = torch.full((D,), 0.5, device=DEV)                                     # accumulated into (+=)
        db = torch.full((1,), 0.5, device=DEV)
        check(lib.rmcl_irtr_bwd(P(dscore), P(cd), I64(D), P(wd), S, D, P(dcls), P(dw), P(db), stream_ptr()))
        torch.cuda.synchronize()
        return scores, dscore, rows, stats, dcls, dw, db

    out = run()
    scores, dscore, rows, stats, dcls, dw, db = out
    c64 = cls.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    z = (c64 @ w64 + b64).view(B, Rr)
    loss = torch.nn.functional.cross_entropy(z, torch.zeros(B, dtype=torch.long))
    (0.125 * loss).backward()
    zs = float(z.detach().abs().max())
    assert float((scores.cpu().double() - z.detach().flatten()).abs().max()) < 1e-5 * max(1.0, zs)
    assert abs(float(stats[0]) - float(loss)) < 1e-5 * max(1.0, float(loss))
    assert float(stats[1]) == float((scores.view(B, Rr).argmax(1) == 0).sum())
    ref_rows = torch.nn.functional.cross_entropy(z.detach(), torch.zeros(B, dtype=torch.long), reduction="none")
    assert float((rows.cpu().double() - ref_rows).abs().max()) < 1e-5 * max(1.0, zs)
    assert float((dcls.cpu().double() - c64.grad).abs().max()) < 1e-6 * max(1.0, float(c64.grad.abs().max()))
    assert float((dw.cpu().double() - 0.5 - w64.grad).abs().max()) < 2e-6 * max(1.0, float(w64.grad.abs().max()))
    assert abs(float(db) - 0.5 - float(b64.grad)) < 2e-6
    for a, c in zip(out, run()):                                                    # fixed reduction order, no float atomics: bit-identical
        assert torch.equal(a, c)
    # data gradient only: no weight-gradient pointers
    dcls2 = torch.empty(S, D, device=DEV)
    check(lib.rmcl_irtr_bwd(P(dscore), P(cd), I64(D), P(wd), S, D, P(dcls2), None, None, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dcls2, dcls)


def test_score_kernel_scatters_through_the_index_and_drops_what_is_outside():
    g = torch.Generator().manual_seed(5)
    S, D, n = 37, 768, 64
    cls, w, b = torch.randn(S, D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV), torch.randn(1, generator=g).to(DEV)
    idx = torch.randperm(n, generator=g)[:S].to(torch.int32)
    idx[3], idx[9] = -1, n + 5                                                      # outside the matrix: dropped
    out = torch.full((n + 8,), 7.0, device=DEV)                                     # 8 guard elements behind the matrix
    check(lib.rmcl_irtr_score(P(cls), I64(D), P(w), P(b), S, D, P(out), P(idx.to(DEV)), I64(n), stream_ptr()))
    torch.cuda.synchronize()
    ref = (cls.double() @ w.double() + b.double()).cpu()
    exp = torch.full((n + 8,), 7.0, dtype=torch.float64)
    for i in range(S):
        if 0 <= int(idx[i]) < n:
            exp[int(idx[i])] = ref[i]
    assert float((out.cpu().double() - exp).abs().max()) < 1e-4
    assert torch.all(out[n:] == 7.0)


# ---- modules ----------------------------------------------------------------------------------------------------------------
def make_module(cfg, p, dtype="f32", **over):
    kw = dict(num_layers=cfg["num_layers"], per_gpu_batchsize=cfg["per_gpu_batchsize"], draw_false_text=cfg["draw_false_text"],
              drop_rate=0.0, max_steps=100, warmup_steps=0, max_image_len=cfg["max_image_len"], get_recall_metric=False)
    kw.update(over)
    m = ViLTransformerSS(task_finetune_irtr_coco(**kw), device=DEV, compute_dtype=dtype)
    sd = {n: t.to(DEV) for n, t in p.items() if not n.startswith(("k_", "moco_head"))}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert sorted(missing) == ["rank_output.bias", "rank_output.weight"] and not unexpected, (missing, unexpected)
    m.train()
    return m


def _run(m, batch, train=True):
    vilt_utils.set_task(m)
    m.zero_grad()
    m.train(train)
    if train:
        ret = m(batch)
        sum(v for k, v in ret.items() if "loss" in k).backward()
    else:
        with torch.no_grad():
            ret = m(batch)
    torch.cuda.synchronize()
    return ret


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_step_matches_reference_golden(name, dtype):
    g = R.load(name)
    cfg, p, batch = R.case_inputs(name)
    tol = TOL[dtype]
    m = make_module(cfg, p, dtype)
    assert m.current_tasks == [] and vilt_utils.set_task(m) is None and m.current_tasks == ["irtr"]      # itm: 0.5 < 1 (vilt_utils.py:325-329)
    ret = _run(m, dev_batch(batch))
    ref = g["irtr_scores"]
    print(name, dtype, "loss", float(ret["irtr_loss"]), float(g["irtr_loss"]), "max score err", float(np.abs(ret["irtr_scores"].cpu().numpy() - ref).max()))
    assert abs(float(ret["irtr_loss"]) - float(g["irtr_loss"])) < tol["loss"] * float(g["irtr_loss"])
    np.testing.assert_allclose(ret["irtr_scores"].cpu().numpy(), ref, atol=tol["logits"] * max(1.0, float(np.abs(ref).max())))
    assert abs(float(m.logged["irtr/train/irtr_loss"]) - float(g["log_irtr__train__irtr_loss"])) < tol["loss"] * float(g["irtr_loss"])
    params = dict(m.named_parameters())
    for n, d in zip(g["grad_names"], g["grad_digest"]):
        got = digest(params[str(n)].grad)
        print("  grad", str(n), got[1], d[1]) if str(n).startswith(("rank_output", "pooler")) else None
        assert abs(got[1] - d[1]) <= tol["grad"] * d[1] + 2e-7, (str(n), got[:3], d[:3])
    for key, t in (("grad_rank_w", params["rank_output.weight"].grad), ("grad_rank_b", params["rank_output.bias"].grad),
                   ("grad_pooler_w", params["pooler.dense.weight"].grad[:8, :64]),
                   ("grad_qkv0_w", params["transformer.blocks.0.attn.qkv.weight"].grad[:8, :64])):
        refg = g[key]
        np.testing.assert_allclose(t.cpu().numpy(), refg, atol=tol["grad"] * 2.5 * np.abs(refg).max() + 2e-7, err_msg=key)
    # the frozen ITM head: no gradient of its own; row 0 of the gradient arena stays zero
    eng = m.engine
    assert params["itm_score.fc.weight"].grad is None and not params["itm_score.fc.weight"].requires_grad
    D = cfg["hidden_size"]
    assert torch.count_nonzero(eng.g32[eng.layout.itm_w:eng.layout.itm_w + D]) == 0 and float(eng.g32[eng.layout.itm_b]) == 0.0
    # validation: the same loss without a backward
    m.logged = {}
    rv = _run(m, dev_batch(batch), train=False)
    assert abs(float(rv["irtr_loss"]) - float(g["irtr_loss"])) < tol["loss"] * float(g["irtr_loss"]) and "irtr/val/irtr_loss" in m.logged


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_steps_move_row_1_with_rank_output_and_leave_row_0(dtype):
    g = R.load(R.TWO_STEP)
    cfg, p, batches = R.two_step_inputs()
    f32 = dtype == "f32"
    m = make_module(cfg, p, dtype, loss_names=_loss_names({"itm": 1, "irtr": 1}), learning_rate=R.LR, weight_decay=R.WD)
    opt = m.configure_optimizers()[0][0]
    assert abs(opt.param_groups[0]["lr"] - R.LR) < 1e-12
    params = dict(m.named_parameters())
    itm_w, itm_b, rank_w, rank_b = (params[k] for k in ("itm_score.fc.weight", "itm_score.fc.bias", "rank_output.weight", "rank_output.bias"))
    assert rank_w.data_ptr() == itm_w[1:].data_ptr() and rank_b.data_ptr() == itm_b[1:].data_ptr()       # views, not copies
    w_init, b_init = itm_w.detach().clone(), itm_b.detach().clone()
    np.testing.assert_array_equal(w_init.cpu().numpy(), g["itm_w_init"])
    sd = m.state_dict()
    assert all(k in sd for k in ("itm_score.fc.weight", "itm_score.fc.bias", "rank_output.weight", "rank_output.bias"))
    eng = m.engine
    D = cfg["hidden_size"]
    for s, batch in enumerate(batches, 1):
        m.itm_labels_override = torch.from_numpy(g[f"s{s}_itm_labels"])
        m.train()
        m.zero_grad()
        loss = m.training_step(dev_batch(batch), s - 1)
        assert m.current_tasks == ["itm", "irtr"]
        loss.backward()
        torch.cuda.synchronize()
        # the ITM loss writes no gradient into the head (nor, through the alias, into rank_output): row 0 and bias 0 stay zero
        assert torch.count_nonzero(eng.g32[eng.layout.itm_w:eng.layout.itm_w + D]) == 0 and float(eng.g32[eng.layout.itm_b]) == 0.0
        tol = TOL[dtype]
        np.testing.assert_allclose(rank_w.grad.cpu().numpy(), g[f"s{s}_grad_rank_w"], atol=tol["grad"] * 2.5 * np.abs(g[f"s{s}_grad_rank_w"]).max())
        if s == 1:
            for n, d in zip(g["grad_names"], g["grad_digest"]):
                got = digest(params[str(n)].grad)
                assert abs(got[1] - d[1]) <= tol["grad"] * d[1] + 2e-7, (str(n), got[:3], d[:3])
        total_ref = float(g[f"s{s}_itm_loss"]) + float(g[f"s{s}_itm_wpa_loss"]) + float(g[f"s{s}_irtr_loss"])
        print("step", s, "loss", float(loss), total_ref)
        assert abs(float(loss) - total_ref) < tol["loss"] * total_ref
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(itm_w[1], rank_w[0]) and torch.equal(itm_b[1:], rank_b)                     # bit for bit
        assert torch.equal(itm_w[0], w_init[0]) and torch.equal(itm_b[0], b_init[0])                   # row 0 frozen, bit for bit
        grads = [g[f"s{t}_grad_rank_w"] for t in range(1, s + 1)]
        undetermined = R.check_adam_row(itm_w[1].detach().cpu().numpy(), g[f"s{s}_itm_w"][1], g["itm_w_init"][1], grads, f"step {s} row 1",
                                        cls=TOL[dtype]["grad"])
        print(dtype, "step", s, "share of row 1 the gradient class leaves undetermined", undetermined)
        R.check_adam_row(itm_b[1:].detach().cpu().numpy(), g[f"s{s}_itm_b"][1:], g["itm_b_init"][1:],
                         [g[f"s{t}_grad_rank_b"] for t in range(1, s + 1)], f"step {s} bias 1", grad_floor=(cfg["draw_false_text"] + 1) * 2.0 ** -23)
        got = digest(params["pooler.dense.weight"])
        assert abs(got[1] - g[f"s{s}_pooler_w_digest"][1]) <= 1e-5 * g[f"s{s}_pooler_w_digest"][1]
        if not f32:
            # the bf16 shadow the GEMMs read follows the masters: row 0 as loaded, row 1 the rounded rank_output
            lp = eng.q_lp[eng.layout.itm_w:eng.layout.itm_w + 2 * D].view(2, D)
            assert torch.equal(lp[0], w_init[0].bfloat16()) and torch.equal(lp[1], rank_w[0].detach().bfloat16())


# ---- recall -----------------------------------------------------------------------------------------------------------------
def _recall_setup(dtype="f32", **over):
    g = R.load(R.RECALL)
    cfg, p, images, iids, ids, masks, tiids = R.recall_inputs()
    m = make_module(cfg, p, dtype, **over)
    m.eval()
    text_dset = [{"text_ids": ids, "text_masks": masks, "img_index": tiids.tolist()}]
    image_dset = [{"image": [img], "img_index": [i]} for img, i in zip(images, iids)]
    return g, cfg, p, m, images, ids, masks, text_dset, image_dset


def test_visual_embed_and_infer_image_embeds_match_the_fixture():
    g, cfg, p, m, images, ids, masks, _, _ = _recall_setup()
    assert m.transformer.visual_embed(images[0].to(DEV))[0].shape == (1, 145, 768)                     # reachable like the reference's
    for i, img in enumerate(images):
        pidx = torch.from_numpy(g[f"img{i}_patch_index"]).long()
        gw = img.shape[3] // cfg["patch_size"]
        sel = (pidx[:, 0] * gw + pidx[:, 1]).view(1, -1)
        emb, msk, (pi, hw), none = m.visual_embed(img.to(DEV), max_image_len=cfg["max_image_len"], select=sel)
        assert none is None and emb.dtype == torch.float32 and tuple(msk.shape) == tuple(emb.shape[:2])
        np.testing.assert_allclose(emb[0][:, ::16].cpu().numpy(), g[f"img{i}_embeds_sub"], atol=2e-5)
        np.testing.assert_allclose(digest(emb[0]), g[f"img{i}_embeds_digest"], rtol=1e-4, atol=1e-4)
        np.testing.assert_array_equal(msk[0].cpu().numpy(), g[f"img{i}_masks"])
        np.testing.assert_array_equal(pi[0].cpu().numpy(), g[f"img{i}_patch_index"])
        assert tuple(hw) == tuple(g[f"img{i}_grid"])
        if i == 0:
            n = ids.shape[0]
            with torch.no_grad():
                out = m.infer({"text_ids": ids.to(DEV), "text_masks": masks.to(DEV)}, image_embeds=emb.expand(n, -1, -1),
                              image_masks=msk.expand(n, -1))
            assert sorted(out) == sorted(["text_feats", "image_feats", "cls_feats", "raw_cls_feats", "image_labels", "image_masks",
                                          "text_labels", "text_ids", "text_masks", "patch_index"])
            np.testing.assert_allclose(out["cls_feats"].cpu().numpy(), g["cls_0"], atol=2e-3)
    with pytest.raises(NotImplementedError):
        m.visual_embed(images[0].to(DEV), mask_it=True)


def test_infer_on_cached_embeds_equals_infer_on_pixels():
    cfg, p, batch = R.case_inputs("irtr_L2_B3_F2_raggedimg")
    m = make_module(cfg, p, "f32")
    m.eval()
    db = dev_batch(batch)
    with torch.no_grad():
        a = m.infer(db)
        emb, msk, _, _ = m.visual_embed(db["image"][0], max_image_len=cfg["max_image_len"])
        b = m.infer(db, image_embeds=emb, image_masks=msk)
    assert torch.equal(a["image_masks"], b["image_masks"])
    for k in ("cls_feats", "raw_cls_feats", "text_feats", "image_feats"):
        scale = float(a[k].abs().max())
        assert float((a[k] - b[k]).abs().max()) <= 1e-4 * scale, k                 # fp32 summation order only
    with pytest.raises(ValueError, match="no_grad"):
        m.infer(db, image_embeds=emb, image_masks=msk)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_score_matrix_does_not_depend_on_the_tiling(dtype):
    g, cfg, p, m, images, ids, masks, text_dset, image_dset = _recall_setup(dtype)
    mats = []
    for ti, tt in ((1, 15), (11, 1), (3, 4), (4, 64)):
        out = objectives.compute_irtr_recall(m, text_dset, image_dset, tile_images=ti, tile_texts=tt, return_scores=True)
        torch.cuda.synchronize()
        assert not torch.isnan(out[6]).any()                                        # every pair scored
        mats.append(out[6].cpu())
    scale = max(1.0, float(mats[0].abs().max()))
    tol = 1e-4 if dtype == "f32" else TOL["bf16"]["logits"]
    for mm in mats[1:]:
        print(dtype, "tiling max diff", float((mm - mats[0]).abs().max()), "scale", scale)
        assert float((mm - mats[0]).abs().max()) <= tol * scale


def test_recall_end_to_end_fp32_equals_the_fixture():
    g, cfg, p, m, images, ids, masks, text_dset, image_dset = _recall_setup("f32")
    rec = objectives.compute_irtr_recall(m, text_dset, image_dset, return_scores=True)
    scores = rec[6].cpu().numpy()
    tol = R.TOL_SCORE_F32 * max(1.0, float(np.abs(g["scores"]).max()))
    print("recall f32 max score err", float(np.abs(scores - g["scores"]).max()), "tol", tol, "min gap", float(g["min_gap"]))
    np.testing.assert_allclose(scores, g["scores"], atol=tol)
    assert [float(x) for x in rec[:6]] == [float(x) for x in g["recalls"]]
    assert rec[7].tolist() == g["iids"].tolist() and rec[8].tolist() == g["tiids"].tolist()
    # epoch_wrapup: the recalls and ir_r1 + tr_r1 in the_metric, at the end of a validation epoch only
    m.hparams.config["get_recall_metric"] = True
    m.irtr_eval_dsets = (text_dset, image_dset)
    out = vilt_utils.epoch_wrapup(m)
    assert [out[f"recalls/{k}"] for k in ("ir_r1", "ir_r5", "ir_r10", "tr_r1", "tr_r5", "tr_r10")] == [float(x) for x in g["recalls"]]
    assert out["the_metric"] == float(g["recalls"][0]) + float(g["recalls"][3])
    m.train()
    assert "the_metric" not in vilt_utils.epoch_wrapup(m)


def test_recall_bf16_scores_in_class():
    g, cfg, p, m, images, ids, masks, text_dset, image_dset = _recall_setup("bf16")
    rec = objectives.compute_irtr_recall(m, text_dset, image_dset, return_scores=True)
    scores = rec[6].cpu().numpy()
    err = float(np.abs(scores - g["scores"]).max())
    print("recall bf16: max score err", err, "recalls", [float(x) for x in rec[:6]], "fixture", g["recalls"].tolist())
    assert err <= TOL["bf16"]["logits"] * max(1.0, float(np.abs(g["scores"]).max()))


# ---- contracts ----------------------------------------------------------------------------------------------------------------
def test_irtr_attacked_is_refused_at_construction():
    with pytest.raises(NotImplementedError, match="text_representation"):
        ViLTransformerSS(task_finetune_irtr_coco(num_layers=2, loss_names=_loss_names({"itm": 0.5, "irtr_attacked": 1})), device=DEV, compute_dtype="f32")


def test_over_long_image_is_refused_before_any_scoring():
    cfg, p, _ = R.case_inputs("irtr_L2_B2_F3")
    m = make_module(cfg, p, "bf16", max_image_len=-1)
    m.eval()
    gen = torch.Generator().manual_seed(3)
    ids, masks, _ = R.synthetic_text(cfg, 10, 9)
    text_dset = [{"text_ids": ids, "text_masks": masks, "img_index": list(range(10))}]
    image_dset = [{"image": [torch.rand(1, 3, 384, 576 if i == 6 else 384, generator=gen) * 2 - 1], "img_index": [i]} for i in range(10)]
    # image 6: 12 x 18 = 216 patches + 1 + 40 = 257 tokens
    with pytest.raises(NotImplementedError, match=r"max_image_len <= 215.*f32"):
        objectives.compute_irtr_recall(m, text_dset, image_dset)
    assert m.engine._rank_pass is None                                              # no rank pass was ever shaped, let alone run
    m2 = make_module(cfg, p, "bf16", max_image_len=215)                            # one of the two ways out
    m2.eval()
    rec = objectives.compute_irtr_recall(m2, text_dset, image_dset, return_scores=True)
    assert rec[6].shape == (10, 10) and torch.isfinite(rec[6]).all()
    with pytest.raises(ValueError, match="at least 10"):
        objectives.irtr_recall_from_scores(rec[6][:4], rec[7][:4], rec[8])


def test_checkpoint_rules(tmp_path):
    """vilt_module.py:134-160 then :233-239 - a training-time load fills itm_score and rank_output follows as its view (the file's own
    rank_output.* are unused); :252-268 - under test_only the file's rank_output.* load after itm_score.* and win on row 1."""
    cfg, p, _ = R.case_inputs("irtr_L2_B2_F3")
    sd = {n: t.clone() for n, t in p.items() if not n.startswith(("k_", "moco_head"))}
    sd["rank_output.weight"] = torch.full((1, cfg["hidden_size"]), 0.5)
    sd["rank_output.bias"] = torch.tensor([0.25])
    path = str(tmp_path / "irtr.ckpt")
    torch.save({"state_dict": sd}, path)
    kw = dict(num_layers=2, per_gpu_batchsize=2, draw_false_text=3, drop_rate=0.0, max_steps=10)
    with pytest.warns(UserWarning):
        m = ViLTransformerSS(task_finetune_irtr_coco(load_path=path, **kw), device=DEV, compute_dtype="f32")
    prm = dict(m.named_parameters())
    assert torch.equal(prm["itm_score.fc.weight"].cpu(), p["itm_score.fc.weight"]) and torch.equal(prm["rank_output.weight"][0].cpu(), p["itm_score.fc.weight"][1])
    assert torch.equal(prm["rank_output.bias"].cpu(), p["itm_score.fc.bias"][1:])
    assert m.load_report["unexpected"] == ["rank_output.bias", "rank_output.weight"]
    m = ViLTransformerSS(task_finetune_irtr_coco(load_path=path, test_only=True, **kw), device=DEV, compute_dtype="f32")
    prm = dict(m.named_parameters())
    assert torch.equal(prm["itm_score.fc.weight"][0].cpu(), p["itm_score.fc.weight"][0])
    assert torch.all(prm["itm_score.fc.weight"][1] == 0.5) and torch.all(prm["rank_output.weight"] == 0.5)
    assert float(prm["itm_score.fc.bias"][1]) == 0.25 and float(prm["itm_score.fc.bias"][0]) == float(p["itm_score.fc.bias"][0])


def test_non_irtr_models_keep_their_state_dict_and_itm_gradients():
    m = ViLTransformerSS(task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=2, loss_names=_loss_names({"moco": 1, "itm": 1})),
                         device=DEV, compute_dtype="f32")
    keys = list(m.state_dict())
    assert not any("rank_output" in k for k in keys) and "itm_score.fc.weight" in keys
    # exactly the keys such a model had before: every spec, the momentum copies of the EMA groups, the queue
    from rmcl_amd.runtime import EMA_GROUPS
    names = [n for n, _, _ in m.engine.specs]
    expected = set(names) | {"k_" + n for n in names if n.split(".")[0] in EMA_GROUPS} | {"proj_queue", "proj_queue_ptr"}
    assert set(keys) == expected and len(keys) == len(expected)
    prm = dict(m.named_parameters())
    assert prm["itm_score.fc.weight"].requires_grad and prm["itm_score.fc.weight"].grad is not None
    assert not m.engine.irtr and m.engine.alias_specs == [] and len(m.engine.specs) == 10 + 12 * 2 + 11
    opt = vilt_utils.FusedAdamW(m, 1e-4, 0.01, 1.0)
    assert opt.seg_end.numel() == len(m.engine.specs)                               # the optimizer groups are the specs, one segment each
    m3 = ViLTransformerSS(task_finetune_irtr_coco(num_layers=2, max_steps=10), device=DEV, compute_dtype="f32")
    opt3 = vilt_utils.FusedAdamW(m3, 1e-4, 0.01, 1.0)
    assert opt3.seg_end.numel() == len(m3.engine.specs) + 1                         # the ITM weight split into row 0 (frozen) and row 1
    with pytest.raises(NotImplementedError):
        m.current_tasks = ["irtr_attacked"]
        m({})
