"""CPU: the VQA oracle (tests/vqa_oracle.py) reproduces every vqa_* golden fixture written from the reference's own compute_vqa /
compute_vqa_attack / PGDAttack_vqa (tools/gen_golden_vqa.py)."""
import numpy as np
import pytest
import torch

from tests import vqa_oracle as V
from tests.golden_util import digest

torch.set_num_threads(8)

HEAD_CROPS = (("grad_vqa_w0", "vqa_classifier.0.weight", (slice(0, 8), slice(0, 64))), ("grad_vqa_b0", "vqa_classifier.0.bias", (slice(0, 64),)),
              ("grad_vqa_g1", "vqa_classifier.1.weight", (slice(0, 64),)), ("grad_vqa_b1", "vqa_classifier.1.bias", (slice(0, 64),)),
              ("grad_vqa_w3", "vqa_classifier.3.weight", (slice(0, 8), slice(0, 64))), ("grad_vqa_b3", "vqa_classifier.3.bias", (slice(0, 64),)),
              ("grad_pooler_w", "pooler.dense.weight", (slice(0, 8), slice(0, 64))),
              ("grad_qkv0_w", "transformer.blocks.0.attn.qkv.weight", (slice(0, 8), slice(0, 64))))


@pytest.fixture(scope="module", params=V.FIXTURES)
def case(request):
    g, cfg, p, batch, targets, attacked = V.load_case(request.param)
    for t in p.values():
        t.requires_grad_(True)
    fn = V.compute_vqa_attack if attacked else V.compute_vqa
    r = fn(p, cfg, batch, targets)
    r["vqa_loss"].backward()
    return g, p, r, targets, attacked


def test_targets_and_labels(case):
    g, p, r, targets, attacked = case
    np.testing.assert_allclose(digest(targets), g["vqa_targets_digest"], rtol=1e-6, atol=1e-6)
    assert g["labels_len"][0] == 0 and 10 in g["labels_len"].tolist()         # an empty row and a row with 10 answers


def test_loss_logits_score(case):
    g, p, r, targets, attacked = case
    task = "vqa_attacked" if attacked else "vqa"
    np.testing.assert_allclose(float(r["vqa_loss"].detach()), float(g["vqa_loss"]), rtol=2e-6)
    np.testing.assert_allclose(r["vqa_logits"].detach().numpy(), g["vqa_logits"], atol=2e-5)
    np.testing.assert_allclose(float(r["vqa_score"]), float(g[f"log_{task}__train__score"]), atol=1e-6)
    np.testing.assert_allclose(float(r["vqa_loss"].detach()), float(g[f"log_{task}__train__loss"]), rtol=2e-6)


ATTACKED = [f for f in V.FIXTURES if "_att_" in f]


@pytest.mark.parametrize("case", ATTACKED, indirect=True)
def test_delta(case):
    g, p, r, targets, attacked = case
    d = r["delta"]
    np.testing.assert_allclose(d[:, :, ::8, ::8].numpy(), g["delta_sub"], atol=1e-7)
    np.testing.assert_allclose(digest(d), g["delta_digest"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(r["delta_log"]), float(g["log_vqa_attacked_attack__train__delta"]), rtol=1e-5)


def test_gradients(case):
    g, p, r, targets, attacked = case
    for key, name, sl in HEAD_CROPS:
        ref = g[key]
        np.testing.assert_allclose(p[name].grad[sl].numpy(), ref, atol=2e-5 * max(1.0, float(np.abs(ref).max())), rtol=2e-3, err_msg=key)
    names = g["grad_names"].tolist()
    for i, n in enumerate(names):
        dg = digest(p[n].grad)
        ref = g["grad_digest"][i]
        np.testing.assert_allclose(dg[1], ref[1], rtol=2e-3, err_msg=n)            # l2 norm of every gradient tensor


@pytest.mark.parametrize("case", ATTACKED, indirect=True)
def test_pgd_leak_is_recorded(case):
    """decision 1: the leaked PGD weight gradients are recorded beside the fixture's gradients, not in them"""
    g, p, r, targets, attacked = case
    a, b = g["grad_digest"][:, 1], g["grad_digest_with_pgd_leak"][:, 1]
    assert np.any(np.abs(a - b) > 1e-3 * np.abs(a))
