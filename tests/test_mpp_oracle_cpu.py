"""CPU: tests/mpp_oracle.py (the restatement of mask_tokens, visual_embed(mask_it=True), MPPHead, compute_mpp and its accuracy) equals
every mpp fixture recorded from the reference's own run (tools/gen_golden_mpp.py), and its seeded masks are reproducible."""
import numpy as np
import pytest
import torch

import rmcl_pkg  # noqa: F401
from tests import mlm_oracle as ML
from tests import mpp_oracle as M
from tests.golden_util import digest


@pytest.mark.parametrize("name", M.FIXTURES)
def test_oracle_equals_the_reference_fixture(name):
    g, cfg, p, batch, masked, replaced, with_mlm_itm = M.load_case(name)
    n = int(g["n"])
    img = batch["image"][0]
    labels = M.image_labels(img, cfg, masked)
    assert np.array_equal(labels.numpy(), g["image_labels"]) and tuple(labels.shape) == (img.shape[0], g["image_labels"].shape[1], 3)
    # the reference's own slot order is a permutation of the row-major one for samples without a pad slot: same labels per patch
    assert np.array_equal(M.image_labels(img, cfg, masked, select=torch.from_numpy(g["ref_select"])).numpy(), g["image_labels_ref"])
    grad_names = [str(x) for x in g["grad_names"]]
    for k in grad_names:
        p[k].requires_grad_(True)
    r = M.compute_mpp(p, cfg, batch, masked, replaced)
    assert r["n"] == n and r["pairs"] == 3 * n
    if n == 0:
        assert np.isnan(float(g["mpp_loss"])) and bool(torch.isnan(r["mpp_loss"]))
        return
    assert abs(float(r["mpp_loss"].detach()) - float(g["mpp_loss"])) < 1e-5 * float(g["mpp_loss"])
    z = r["mpp_rows"].detach()
    assert float(np.abs(z.numpy() - g["row_logits"]).max()) < 2e-4 * max(1.0, float(g["zmax"]))
    assert np.array_equal(z.reshape(n, 3, 256).argmax(2).numpy(), g["argmax"]) and r["correct"] == int(g["correct"])
    assert abs(r["correct"] / (3 * n) - float(g["log_accuracy"])) < 1e-6
    loss = r["mpp_loss"]
    if with_mlm_itm:
        r1 = ML.compute_mlm(p, cfg, batch)
        from oracle import rmcl_oracle as O
        r2 = O.compute_itm_wpa(p, cfg, batch, torch.from_numpy(g["itm_labels"]))
        loss = loss + r1["mlm_loss"] + r2["itm_loss"] + r2["itm_wpa_loss"]
        assert abs(float(loss.detach()) - float(g["total_loss"])) < 1e-4 * float(g["total_loss"])
    loss.backward()
    for k, d in zip(grad_names, g["grad_digest"]):
        got = digest(p[k].grad)
        assert abs(got[1] - d[1]) <= 2e-3 * d[1] + 1e-7, (k, got[1], d[1])
    assert float(np.abs(p["transformer.mask_token"].grad.flatten().numpy() - g["grad_mask_token"]).max()) < 2e-3 * float(np.abs(g["grad_mask_token"]).max())


def test_seeded_masks_are_reproducible_and_cover_the_edge_cases():
    g, cfg, p, batch, masked, replaced, _ = M.load_case("mpp_L2_B4_ragged")
    img = batch["image"][0]
    a = M.make_masks(img, cfg, 181, "ragged")
    b = M.make_masks(img, cfg, 181, "ragged")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], masked) and torch.equal(a[1], replaced)     # what the reference was handed
    sel, valid = M.selection(img, cfg)
    mk = torch.gather(masked, 1, sel)
    rp = torch.gather(replaced, 1, sel)
    assert not bool(mk[0].any())                                          # a sample with no masked patch
    c1 = int(valid[1].sum())
    assert bool(mk[1, 0]) and bool(mk[1, c1 - 1])                         # first and last valid slot
    pads = ~valid
    assert bool((mk & pads).any())                                        # a masked pad slot ...
    lab = M.image_labels(img, cfg, masked)[:, 1:]
    assert bool((lab[pads] == -100).all())                                # ... that carries no label
    assert bool((mk & ~rp & valid).any())                                 # masked but not replaced: keeps its embedding, carries a label
    e = M.make_masks(img, cfg, 5, "empty")
    assert not bool(e[0].any()) and not bool(e[1].any())
