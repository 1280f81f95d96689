"""CPU: the NLVR2 oracle (tests/nlvr2_oracle.py) reproduces every nlvr2_* golden fixture written from the reference's own compute_nlvr2 /
compute_nlvr2_attack / PGDAttack_nlvr2 (tools/gen_golden_nlvr2.py): losses, logits, both deltas (and the zero delta of an image that is
not attacked), gradient digests and the logged values."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import nlvr2_oracle as N
from tests.golden_util import digest

torch.set_num_threads(8)

CROPS = (("grad_nlvr2_w0", "nlvr2_classifier.0.weight", (slice(0, 8), slice(0, 64))), ("grad_nlvr2_b0", "nlvr2_classifier.0.bias", (slice(0, 64),)),
         ("grad_nlvr2_g1", "nlvr2_classifier.1.weight", (slice(0, 64),)), ("grad_nlvr2_w3", "nlvr2_classifier.3.weight", (slice(None), slice(0, 64))),
         ("grad_nlvr2_b3", "nlvr2_classifier.3.bias", (slice(None),)), ("grad_token_type", "token_type_embeddings.weight", (slice(None),)),
         ("grad_pooler_w", "pooler.dense.weight", (slice(0, 8), slice(0, 64))),
         ("grad_qkv0_w", "transformer.blocks.0.attn.qkv.weight", (slice(0, 8), slice(0, 64))))


@pytest.fixture(scope="module", params=N.FIXTURES)
def case(request):
    g, cfg, p, batch, idx = N.load_case(request.param)
    for t in p.values():
        t.requires_grad_(True)
    if idx is None:
        r = N.compute_nlvr2(p, cfg, batch)
        r["nlvr2_loss"].backward()
    else:
        r = N.compute_nlvr2_attack(p, cfg, batch, idx)
        (r["nlvr2_original_loss"] + r["nlvr2_attacked_loss"]).backward()
    return g, p, r, batch, idx


def test_losses_and_logits(case):
    g, p, r, batch, idx = case
    assert g["answers"].tolist() == [int(a) for a in batch["answers"]]
    keys = ("nlvr2_loss",) if idx is None else ("nlvr2_original_loss", "nlvr2_attacked_loss")
    for k in keys:
        np.testing.assert_allclose(float(r[k].detach()), float(g[k]), rtol=2e-6, err_msg=k)
        lk = k.replace("_loss", "_logits")
        np.testing.assert_allclose(r[lk].detach().numpy(), g[lk], atol=2e-6, err_msg=lk)
    if idx is None:
        np.testing.assert_allclose(float(r["nlvr2_loss"].detach()), float(g["log_nlvr2__train__loss"]), rtol=2e-6)


def test_third_token_type_row_differs_from_the_second(case):
    g, p, r, batch, idx = case
    tt = p["token_type_embeddings.weight"].detach()
    assert tt.shape[0] == 3 and float((tt[2] - tt[1]).abs().max()) > 0.05
    assert float(np.abs(g["grad_token_type"][1]).max()) > 0 and float(np.abs(g["grad_token_type"][2]).max()) > 0


ATTACKED = [f for f in N.FIXTURES if "_att_" in f]


@pytest.mark.parametrize("case", ATTACKED, indirect=True)
def test_deltas_and_logs(case):
    g, p, r, batch, idx = case
    for k in range(2):
        d = r[f"delta{k}"]
        np.testing.assert_allclose(d[:, :, ::8, ::8].numpy(), g[f"delta{k}_sub"], atol=1e-7)
        np.testing.assert_allclose(digest(d), g[f"delta{k}_digest"], rtol=1e-5, atol=1e-6)
        if not idx[k]:
            assert not np.any(g[f"delta{k}_sub"]) and float(d.abs().max()) == 0.0
    np.testing.assert_allclose(float(r["delta_log"]), float(g["log_nlvr2_attacked_attack__val__delta"]), rtol=1e-5)
    lab = r["nlvr2_labels"]
    for split, rows in (("dev", [0, 1]), ("test", [2, 3])):
        for kind, lg in (("original", r["nlvr2_original_logits"]), ("attacked", r["nlvr2_attacked_logits"])):
            lg = lg.detach()
            np.testing.assert_allclose(float(F.cross_entropy(lg[rows], lab[rows])), float(g[f"log_nlvr2_{kind}__{split}__loss"]), rtol=2e-6)
            assert float((lg[rows].argmax(1) == lab[rows]).float().mean()) == float(g[f"log_nlvr2_{kind}__{split}__accuracy"])
        chg = (r["nlvr2_attacked_logits"][rows].argmax(1) != r["nlvr2_original_logits"][rows].argmax(1)).float().mean()
        assert float(chg) == float(g[f"log_nlvr2_attacked__{split}__change_rate_cross"])


def test_gradients(case):
    g, p, r, batch, idx = case
    for key, name, sl in CROPS:
        ref = g[key]
        np.testing.assert_allclose(p[name].grad[sl].numpy(), ref, atol=2e-5 * max(1.0, float(np.abs(ref).max())), rtol=2e-3, err_msg=key)
    for i, n in enumerate(g["grad_names"].tolist()):
        np.testing.assert_allclose(digest(p[n].grad)[1], g["grad_digest"][i][1], rtol=2e-3, err_msg=n)
