"""CPU: the image-text retrieval oracle (tests/irtr_oracle.py) reproduces every irtr* golden fixture written from the reference's own
compute_irtr / compute_itm_wpa / compute_irtr_recall (tools/gen_golden_irtr.py): losses, scores, gradient digests, the alias of the
two-step fixture (row 1 of the ITM head moves with rank_output, row 0 does not move) and the recall score matrix with its six values."""
import numpy as np
import pytest
import torch

from tests import irtr_oracle as R
from tests.golden_util import digest

torch.set_num_threads(8)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_step_fixture(name):
    g = R.load(name)
    cfg, p, batch = R.case_inputs(name)
    w = p["itm_score.fc.weight"][1:].clone().requires_grad_(True)
    b = p["itm_score.fc.bias"][1:].clone().requires_grad_(True)
    for n, t in p.items():
        t.requires_grad_(not n.startswith("itm_score"))
    r = R.compute_irtr(p, cfg, batch, w, b)
    r["irtr_loss"].backward()
    np.testing.assert_allclose(float(r["irtr_loss"]), float(g["irtr_loss"]), rtol=2e-6)
    np.testing.assert_allclose(float(g["log_irtr__train__irtr_loss"]), float(g["irtr_loss"]), rtol=1e-7)
    np.testing.assert_allclose(r["irtr_scores"].detach().numpy(), g["irtr_scores"], atol=2e-6)
    assert g["irtr_scores"].shape == (batch["image"][0].shape[0], cfg["draw_false_text"] + 1)
    grads = {n: t.grad for n, t in p.items() if t.grad is not None}
    grads["rank_output.weight"], grads["rank_output.bias"] = w.grad, b.grad
    names = g["grad_names"].tolist()
    assert "rank_output.weight" in names and "rank_output.bias" in names and not any(n.startswith("itm_score") for n in names)
    for i, n in enumerate(names):
        # (rank_output.bias: the sum of softmax - onehot is zero up to rounding, hence the absolute term)
        np.testing.assert_allclose(digest(grads[n])[1], g["grad_digest"][i][1], rtol=2e-3, atol=2e-7, err_msg=n)
    for key, t in (("grad_rank_w", w.grad), ("grad_rank_b", b.grad), ("grad_pooler_w", grads["pooler.dense.weight"][:8, :64]),
                   ("grad_qkv0_w", grads["transformer.blocks.0.attn.qkv.weight"][:8, :64])):
        ref = g[key]
        np.testing.assert_allclose(t.numpy(), ref, atol=2e-3 * float(np.abs(ref).max()) + (2e-7 if key == "grad_rank_b" else 1e-9), err_msg=key)


def test_two_step_alias():
    g = R.load(R.TWO_STEP)
    cfg, p, batches = R.two_step_inputs()
    labels = [torch.from_numpy(g[f"s{s}_itm_labels"]) for s in (1, 2)]
    out = R.two_steps(p, cfg, batches, labels)
    w0 = g["itm_w_init"]
    np.testing.assert_array_equal(w0, p["itm_score.fc.weight"].numpy())
    for s, (w, b, losses) in enumerate(out, 1):
        for k, v in losses.items():
            # step 2 runs on weights one Adam step apart: its ill-conditioned elements (R.check_adam_row) shift the loss: the fp32 loss class
            np.testing.assert_allclose(v, float(g[f"s{s}_{k}"]), rtol=2e-5 if s == 1 else 1e-3, atol=2e-7 if s == 1 else 1e-5, err_msg=f"step {s} {k}")
        # the fixture itself: the alias (bit for bit) and the frozen row
        np.testing.assert_array_equal(g[f"s{s}_itm_w"][1], g[f"s{s}_rank_w"][0])
        np.testing.assert_array_equal(g[f"s{s}_itm_b"][1:], g[f"s{s}_rank_b"])
        np.testing.assert_array_equal(g[f"s{s}_itm_w"][0], w0[0])
        np.testing.assert_array_equal(g[f"s{s}_itm_b"][0], g["itm_b_init"][0])
        # the oracle's step: Adam's first steps move every element by about lr, in the direction of its gradient
        np.testing.assert_array_equal(w[0].numpy(), w0[0])
        moved = g[f"s{s}_itm_w"][1] - w0[1]
        assert 0.5 * s * R.LR < float(np.abs(moved).mean()) < 1.1 * s * R.LR
        R.check_adam_row(w[1].numpy(), g[f"s{s}_itm_w"][1], w0[1], [g[f"s{t}_grad_rank_w"] for t in range(1, s + 1)], f"step {s} row 1")
        assert float(b[0]) == float(g["itm_b_init"][0])
        # the bias gradient is analytically zero (softmax - onehot sums to 0): rounding noise, so Adam may move it by up to lr per step
        R.check_adam_row(b[1:].numpy(), g[f"s{s}_itm_b"][1:], g["itm_b_init"][1:], [g[f"s{t}_grad_rank_b"] for t in range(1, s + 1)], f"step {s} bias 1",
                         grad_floor=(cfg["draw_false_text"] + 1) * 2.0 ** -23)


def test_recall_fixture():
    g = R.load(R.RECALL)
    cfg, p, images, iids, ids, masks, tiids = R.recall_inputs()
    assert g["iids"].tolist() == iids and g["tiids"].tolist() == tiids.tolist() and len(images) == 11 and len(tiids) == 15
    selects = []
    for i, img in enumerate(images):
        pidx = torch.from_numpy(g[f"img{i}_patch_index"]).long()
        gw = img.shape[3] // cfg["patch_size"]
        sel = (pidx[:, 0] * gw + pidx[:, 1]).view(1, -1)
        selects.append(sel)
        ie, im, _ = R.visual_embed(p, cfg, img, sel)
        np.testing.assert_allclose(ie[0][:, ::16].numpy(), g[f"img{i}_embeds_sub"], atol=2e-5)      # K = 3072 fp32 dot products, order differs
        np.testing.assert_allclose(digest(ie[0]), g[f"img{i}_embeds_digest"], rtol=1e-5, atol=1e-5)
        np.testing.assert_array_equal(im[0].numpy(), g[f"img{i}_masks"])
        assert tuple(g[f"img{i}_grid"]) == (img.shape[2] // 32, img.shape[3] // 32)
    assert len({tuple(im.shape[2:]) for im in images}) == 5
    with torch.no_grad():
        scores = R.score_matrix(p, cfg, images, selects, ids, masks)
    tol = R.TOL_SCORE_F32 * max(1.0, float(np.abs(g["scores"]).max()))
    np.testing.assert_allclose(scores.numpy(), g["scores"], atol=0.05 * tol)
    assert float(g["min_gap"]) >= 20 * tol
    rec = R.recall_from_scores(scores, torch.tensor(iids), tiids)
    assert [float(x) for x in rec] == [float(x) for x in g["recalls"]]
