"""CPU: the prediction fixture tests/golden/predict_L2.npz (tools/gen_golden_predict.py: the reference's own model and heads) against the
CPU oracle (oracle.rmcl_oracle + tests/mlm_oracle.py + tests/vqa_oracle.py through tests/predict_oracle.py), decision by decision; the
margins stored in the fixture; and the argument errors of ``rmcl_amd.Predictor`` and ``Engine.rows_topk`` that need no GPU."""
import types

import numpy as np
import pytest
import torch

from oracle import rmcl_oracle as O
from tests import predict_oracle as PO
from tests import vqa_oracle as V
from tests.golden_util import load


@pytest.fixture(scope="module")
def fixture():
    return load(PO.FIXTURE)


@pytest.fixture(scope="module", params=PO.CASES)
def case(request, fixture):
    """one case with the oracle's own run of the loop (computed once, shared)"""
    cfg, p, batch, order = PO.load_case(fixture, request.param)
    torch.set_num_threads(8)
    with torch.no_grad():
        final, rounds = PO.fill_loop(PO.oracle_logits_fn(p, cfg, batch), batch["text_ids"], batch["text_masks"])
    return types.SimpleNamespace(name=request.param, g=fixture, cfg=cfg, p=p, batch=batch, order=order, final=final, rounds=rounds)


def test_fixture_describes_the_seeded_batch(case):
    g, n = case.g, case.name
    assert np.array_equal(g[f"{n}_ids0"], case.batch["text_ids"].numpy()) and np.array_equal(g[f"{n}_masks"], case.batch["text_masks"].numpy())
    assert [int((r == PO.MASK_ID).sum()) for r in g[f"{n}_ids0"]] == list(PO.N_MASKS)
    lens = g[f"{n}_masks"].sum(axis=1)
    assert (len(set(lens.tolist())) > 1) == (n == "ragged")                # the ragged case has unequal text lengths
    assert g[f"{n}_ids0"].max() < PO.WORD1                                 # the toy vocabulary
    assert [int(x) for x in g["meta"]] == [PO.SEEDS[k] for k in ("weights", "mlm_head", "vqa_head", "batch", "design")]


def test_oracle_reproduces_every_recorded_decision(case):
    g, n = case.g, case.name
    fills = [(r, f["sentence"], f["position"], f["token"]) for r, this in enumerate(case.rounds) for f in this]
    assert fills == [tuple(int(v) for v in row) for row in g[f"{n}_fills"]]
    assert len(fills) == sum(PO.N_MASKS) and len(case.rounds) == max(PO.N_MASKS)
    assert [[f[2] for f in fills if f[1] == b] for b in range(PO.B)] == case.order          # the prescribed order, not left to right
    flat = [f for this in case.rounds for f in this]
    assert np.array_equal(np.array([f["top_ids"] for f in flat]), g[f"{n}_top_ids"])           # the top-5 order of every fill
    assert np.array_equal(case.final.numpy(), g[f"{n}_final_ids"])
    ids0 = g[f"{n}_ids0"]
    assert np.array_equal(case.final.numpy()[0], ids0[0])                                       # the sentence without masks is unchanged
    assert np.array_equal(case.final.numpy() != ids0, ids0 == PO.MASK_ID)                        # only masked positions changed
    # probabilities: the oracle's fp32 logits against the reference's, through the softmax (fp32 contract of the logits 2e-3 |z|max:
    # log p moves by at most twice that)
    e = 2e-3 * float(g[f"{n}_margins"][2])
    bound = np.expm1(2 * e)
    assert np.all(np.abs(np.array([f["top_probs"] for f in flat]) - g[f"{n}_top_probs"]) <= bound * g[f"{n}_top_probs"] + 1e-300)
    assert np.all(np.abs(np.array([f["prob"] for f in flat]) - g[f"{n}_fill_prob"]) <= bound * g[f"{n}_fill_prob"])


def test_margins_of_the_fixture_leave_no_decision_to_skip(case):
    g, n = case.g, case.name
    rank_gap, pos_gap, zmax = (float(v) for v in g[f"{n}_margins"])
    need = PO.MARGIN_FACTOR * PO.BF16_LOGITS_TOL * max(1.0, zmax)
    assert rank_gap >= need and pos_gap >= need, (rank_gap, pos_gap, need)
    got = PO.margins(case.rounds)                                                               # the oracle finds the same margins
    assert abs(got[0] - rank_gap) < 1e-2 and abs(got[1] - pos_gap) < 1e-2 and abs(got[2] - zmax) < 1e-2
    vgap, vzmax = (float(v) for v in g[f"{n}_vqa_margins"])
    assert vgap >= PO.MARGIN_FACTOR * PO.BF16_LOGITS_TOL * max(1.0, vzmax)
    assert float(np.linalg.norm(g[f"{n}_mlm_rows"], axis=1).max()) < 8.0                         # the designed rows stay ordinary in size


def test_oracle_reproduces_the_vqa_answers(case):
    g, n = case.g, case.name
    with torch.no_grad():
        out = O.infer(case.p, case.cfg, case.batch["text_ids"], case.batch["text_masks"], case.batch["image"][0])
        z = V.vqa_head(case.p, out["cls_feats"])
    top = z.topk(PO.TOP_K, dim=1)
    assert np.array_equal(top.indices.numpy(), g[f"{n}_vqa_top_ids"])
    assert np.array_equal(z.argmax(dim=1).numpy(), g[f"{n}_vqa_top_ids"][:, 0])
    assert np.abs(top.values.numpy() - g[f"{n}_vqa_top_logits"]).max() <= 2e-3 * float(g[f"{n}_vqa_margins"][1])


# ---- argument errors that need no GPU ----------------------------------------------------------------------------------------------------
def _predictor(**heads):
    import rmcl_pkg  # noqa: F401
    from rmcl_amd import Predictor
    eng = types.SimpleNamespace(cfg={"max_text_len": 40}, mlm=heads.get("mlm"), vqa=heads.get("vqa"), device=torch.device("cpu"))
    return Predictor, types.SimpleNamespace(engine=eng, id2answer=None)


def test_predictor_is_exported_and_loads_local_tokenizers_only():
    Predictor, model = _predictor()
    import rmcl_amd
    from rmcl_amd.predict import Predictor as P2
    assert rmcl_amd.Predictor is P2 is Predictor
    with pytest.raises(ValueError, match="nothing is fetched"):
        Predictor(model, tokenizer="bert-base-uncased")                    # a hub name: never fetched
    pr = Predictor(model, tokenizer=PO.VOCAB)
    assert pr.tokenizer.mask_token_id == PO.MASK_ID
    ids, masks = pr._encode(["a [MASK] on the", "the"])
    assert tuple(ids.shape) == (2, 40) and int(ids[0, 2]) == PO.MASK_ID and int(masks[1].sum()) == 3
    assert Predictor(model, id2answer={3: "yes"}).id2answer == {3: "yes"}


def test_predictor_argument_errors():
    Predictor, model = _predictor()
    pr = Predictor(model)
    img = torch.zeros(3, 32, 32)
    batch = {"text_ids": torch.zeros(1, 40, dtype=torch.int64), "text_masks": torch.ones(1, 40, dtype=torch.int64), "image": [img[None]]}
    with pytest.raises(ValueError, match=r"loss_names\['mlm'\] > 0"):
        pr.mlm_topk(batch)
    with pytest.raises(ValueError, match=r"loss_names\['mlm'\] > 0"):
        pr.fill_mask(img, text_ids=batch["text_ids"], mask_token_id=103)
    with pytest.raises(ValueError, match=r"loss_names\['vqa'\] > 0"):
        pr.answer(batch)
    Predictor, model = _predictor(mlm=object(), vqa=types.SimpleNamespace(N=3129))
    pr = Predictor(model)
    with pytest.raises(ValueError, match="mask id"):
        pr.fill_mask(img, text_ids=batch["text_ids"])                      # no tokenizer and no mask_token_id
    with pytest.raises(ValueError, match="needs a tokenizer"):
        pr.fill_mask(img, text="a [MASK]", mask_token_id=103)
    with pytest.raises(ValueError, match="either text"):
        pr.fill_mask(img, mask_token_id=103)
    with pytest.raises(ValueError, match="either text"):
        pr.fill_mask(img, text="a", text_ids=batch["text_ids"], mask_token_id=103)
    with pytest.raises(ValueError, match="max_text_len"):
        pr.fill_mask(img, text_ids=torch.zeros(1, 12, dtype=torch.int64), mask_token_id=103)
    with pytest.raises(ValueError, match="top_k"):
        pr.fill_mask(img, text_ids=batch["text_ids"], mask_token_id=103, top_k=33)
    with pytest.raises(ValueError, match="top_k"):
        pr.answer(batch, top_k=0)
    with pytest.raises(ValueError, match="needs a tokenizer"):
        pr.answer((img, "what is on the table"))
    with pytest.raises(ValueError, match="image must be"):
        pr._image(torch.zeros(32, 32))
    with pytest.raises(ValueError, match="2 images for 3 texts"):
        pr._image(torch.zeros(2, 3, 32, 32), 3)
    s = torch.zeros(12, 15)
    with pytest.raises(ValueError, match=r"\[images, captions\]"):
        pr.retrieve(s, torch.arange(12), torch.arange(14))
    with pytest.raises(ValueError, match="k must be"):
        pr.retrieve(s, torch.arange(12), torch.arange(15), k=13)
    with pytest.raises(ValueError, match="R@10"):
        pr.recall(torch.zeros(9, 15), torch.arange(9), torch.arange(15))


def test_engine_rows_topk_argument_errors():
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.runtime import Engine
    f = lambda *a, **k: Engine.rows_topk(None, *a, **k)                      # the checks precede every use of the engine
    x = torch.zeros(4, 8)
    for args, kw, what in (((x, 2), dict(mode="max"), "mode must be"), ((x, 2), dict(want_lse=True), "want_lse"), ((x.double(), 2), {}, "2-D fp32"),
                           ((x[0], 2), {}, "2-D fp32"), ((x, 2), {}, "on the device")):
        with pytest.raises(ValueError, match=what):
            f(*args, **kw)
