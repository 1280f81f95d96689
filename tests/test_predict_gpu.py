"""-m gpu: ``rmcl_amd.Predictor`` - mask filling, masked-token candidates, VQA answers, retrieval lists - and ``Engine.rows_topk``.

Fixture tests/golden/predict_L2.npz (tools/gen_golden_predict.py: the reference's own model and heads; tests/predict_oracle.py): every
recorded decision must come out the same on the fp32 AND on the bf16 engine - the filled position of every round, its token, the order of
its top five, the VQA answers.  In the sentence with four masks the three certain positions (fp32 probability exactly 1.0: a tie) must go
from left to right and the leftmost, uncertain position last (tests/predict_oracle.py).  No decision is skipped: the generator refused
any margin below twice the bf16 logits tolerance of tests/test_mlm_gpu.py (0.1 * max(1, |z|max)), so an engine inside that tolerance
cannot legitimately decide otherwise.
Probabilities, fp32 engine: tests/test_mlm_gpu.py holds fp32 logits to e = 2e-3 * max(1, |z|max) of the reference.  log p_i = z_i - lse(z)
moves by at most 2e when every logit moves by at most e, so |p - p_ref| <= p_ref * (exp(2e) - 1): 0.155 p_ref at |z|max = 36.1.  The
largest observed |p - p_ref| / p_ref goes to the file named by RMCL_PREDICT_PARITY_OUT when set (profiles/predict_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd import Predictor  # noqa: E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd.vilt.config import task_mlm_itm, task_finetune_vqa, task_moco, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, objectives  # noqa: E402
from tests import mlm_oracle as M  # noqa: E402
from tests import predict_oracle as PO  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402
from tests import topk_ref as T  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"
FP32_LOGITS_TOL = 2e-3                     # tests/test_mlm_gpu.py TOL["f32"]["logits"] (x max(1, |z|max))
OBSERVED = {}


@pytest.fixture(scope="module", autouse=True)
def parity_dump():
    yield
    out = os.environ.get("RMCL_PREDICT_PARITY_OUT")
    if out and OBSERVED:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec["predictor"] = {"what": "fill_mask / answer on tests/golden/predict_L2.npz: largest |p - p_ref| / p_ref of the recorded top-5 probabilities "
                                    "(bound on the fp32 engine: exp(2 * 2e-3 * |z|max) - 1) and |logit - ref| / |z|max of the VQA top-5", **OBSERVED}
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


def make_module(p, dtype, B=PO.B, drop_rate=0.0, vqa=True):
    cfg = task_mlm_itm(num_layers=2, per_gpu_batchsize=B, drop_rate=drop_rate, max_steps=100, warmup_steps=0,
                       loss_names=_loss_names({"mlm": 1, "vqa": int(vqa)}))
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype=dtype)
    skip = ("k_", "moco_head", "itm_score") + (() if vqa else ("vqa_classifier",))
    missing, unexpected = m.load_state_dict({n: t.to(DEV) for n, t in p.items() if not n.startswith(skip)}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return m


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", PO.CASES)
def test_fixture_decisions_are_reproduced(case, dtype):
    g = load(PO.FIXTURE)
    cfg, p, batch, order = PO.load_case(g, case)
    m = make_module(p, dtype)
    m.train()
    eng = m.engine
    state = ([mod.training for mod in m.modules()], eng.dropout_on, eng.pass_counter)
    pr = Predictor(m, tokenizer=PO.VOCAB, id2answer=[f"answer {i}" for i in range(3129)])
    res = pr.fill_mask(batch["image"][0], text_ids=batch["text_ids"], text_masks=batch["text_masks"], top_k=PO.TOP_K)
    assert ([mod.training for mod in m.modules()], eng.dropout_on, eng.pass_counter) == state and torch.is_grad_enabled()
    fills = g[f"{case}_fills"]
    zmax = float(g[f"{case}_margins"][2])
    bound = float(np.expm1(2 * FP32_LOGITS_TOL * max(1.0, zmax)))
    worst = 0.0
    for b in range(PO.B):
        rows = [j for j in range(len(fills)) if int(fills[j, 1]) == b]                  # this sentence's fills, in round order
        got = res["fills"][b]
        assert [(f["position"], f["token_id"]) for f in got] == [(int(fills[j, 2]), int(fills[j, 3])) for j in rows], (case, dtype, b)
        for f, j in zip(got, rows):
            assert f["top_ids"] == g[f"{case}_top_ids"][j].tolist(), (case, dtype, b, j)
            assert f["token"] == pr.tokenizer.convert_ids_to_tokens([f["token_id"]])[0] and len(f["top_tokens"]) == PO.TOP_K
            ref = g[f"{case}_top_probs"][j]
            rel = np.abs(np.array(f["top_probs"], dtype=np.float64) - ref) / np.maximum(ref, 1e-300)
            rel = rel[ref > 1e-30]                                                      # (places whose fp32 probability is a denormal or 0)
            worst = max(worst, float(rel.max()))
            if dtype == "f32":
                assert rel.max() <= bound, (case, b, j, f["top_probs"], ref.tolist(), bound)
            assert abs(f["prob"] - f["top_probs"][0]) == 0.0
    OBSERVED[f"fill_mask_{case}_{dtype}"] = {"largest_rel_prob_error": worst, "fp32_bound": bound}
    assert np.array_equal(res["ids"].numpy(), g[f"{case}_final_ids"])
    assert np.array_equal(res["ids"][0].numpy(), g[f"{case}_ids0"][0]) and res["fills"][0] == []       # no mask: unchanged
    assert len(res["text"]) == PO.B and "[MASK]" not in " ".join(res["text"])
    assert res["text"][2] == pr.tokenizer.decode(g[f"{case}_final_ids"][2][g[f"{case}_masks"][2] != 0].tolist(), skip_special_tokens=True)
    # the same loop from text: one tokenisation, one decoding
    text = [pr.tokenizer.decode(r[mk != 0][1:-1].tolist()) for r, mk in zip(g[f"{case}_ids0"], g[f"{case}_masks"])]
    again = pr.fill_mask(batch["image"][0], text=text, top_k=1)
    valid = g[f"{case}_masks"] != 0
    assert np.array_equal(again["ids"].numpy()[valid], g[f"{case}_final_ids"][valid])
    # VQA answers of the same batch
    ans = pr.answer(dev_batch(batch), top_k=PO.TOP_K)
    assert np.array_equal(ans["ids"].cpu().numpy(), g[f"{case}_vqa_top_ids"]), (case, dtype)
    vz = float(g[f"{case}_vqa_margins"][1])
    zerr = float(np.abs(ans["logits"].cpu().numpy() - g[f"{case}_vqa_top_logits"]).max()) / vz
    OBSERVED[f"answer_{case}_{dtype}"] = {"largest_logit_error_over_zmax": zerr}
    assert zerr <= (FP32_LOGITS_TOL if dtype == "f32" else PO.BF16_LOGITS_TOL)
    assert torch.equal(ans["scores"], torch.sigmoid(ans["logits"])) or float((ans["scores"] - torch.sigmoid(ans["logits"])).abs().max()) < 1e-6
    assert ans["answers"][1][0] == f"answer {int(g[f'{case}_vqa_top_ids'][1, 0])}"
    assert ([mod.training for mod in m.modules()], eng.dropout_on, eng.pass_counter) == state


def test_mlm_topk_agrees_with_the_heads_argmax_and_the_model():
    g = load(PO.FIXTURE)
    cfg, p, batch, _ = PO.load_case(g, "ragged")
    m = make_module(p, "f32", vqa=False)
    m.eval()
    pr = Predictor(m)
    db = dev_batch(batch)
    ids1, p1 = pr.mlm_topk(db, k=1)
    ids5, p5 = pr.mlm_topk(db, k=5)
    Lt = cfg["max_text_len"]
    assert tuple(ids1.shape) == (PO.B, Lt, 1) and tuple(p5.shape) == (PO.B, Lt, 5) and ids5.dtype == torch.int64
    ma = m.engine.mlm_bufs(PO.B, "predict")
    assert torch.equal(ids1.view(-1).to(torch.int32), ma.argmax[: PO.B * Lt])           # what mlm_forward wrote for the same rows
    assert torch.equal(ids5[:, :, :1], ids1) and torch.equal(p5[:, :, :1], p1)
    assert not m.training
    # against the dense logits of the public path (eval, no_grad): the float64 model of the kernel on every row
    out = m.validation_step(dict(db, text_ids_mlm=db["text_ids"], text_labels_mlm=torch.full_like(db["text_ids"], -100)), 0)
    z = out["mlm_logits"].view(PO.B * Lt, -1).cpu().numpy()
    wi, _, wp, _ = T.rows_topk(z, 5, "softmax")
    assert np.array_equal(ids5.view(-1, 5).cpu().numpy(), wi)
    for r in (0, Lt + 3, 2 * Lt + 7):
        assert np.all(np.abs(p5.view(-1, 5)[r].cpu().numpy() - wp[r]) <= T.prob_allowance(z[r], z[r, wi[r]], wp[r], "softmax"))


def test_answer_is_vqa_preds_at_full_width_and_in_chunks():
    B = 257                                                                               # one more than the head launcher takes
    m = ViLTransformerSS(task_finetune_vqa(num_layers=1, per_gpu_batchsize=B, drop_rate=0.0), device=DEV, compute_dtype="f32")
    gen = torch.Generator().manual_seed(9)
    ids = torch.randint(1000, 30522, (B, 40), generator=gen)
    ids[:, 0], ids[:, -1] = 101, 102
    batch = {"text_ids": ids.to(DEV), "text_masks": torch.ones(B, 40, dtype=torch.int64, device=DEV),
             "image": [(torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1).to(DEV)]}
    names = [f"a{i}" for i in range(3129)]
    pr = Predictor(m, id2answer=names)
    ans = pr.answer(batch, top_k=1)
    ans3 = pr.answer(batch, top_k=3)
    assert tuple(ans["ids"].shape) == (B, 1) and m.engine.vqa.N == 3129
    preds, logits = [], []
    m.eval()
    for s, e in ((0, 256), (256, 257)):
        part = {"text_ids": batch["text_ids"][s:e], "text_masks": batch["text_masks"][s:e], "image": [batch["image"][0][s:e]],
                "vqa_labels": [[] for _ in range(e - s)], "vqa_scores": [[] for _ in range(e - s)]}
        out = m.validation_step(part, 0)
        preds.append(out["vqa_preds"].clone())
        logits.append(out["vqa_logits"].clone())
    preds, logits = torch.cat(preds).to(torch.int64), torch.cat(logits)
    assert tuple(logits.shape) == (B, 3129)
    assert torch.equal(ans["ids"][:, 0], preds) and torch.equal(ans3["ids"][:, 0], preds)
    # every row is its own question's: the best logit of row b is the maximum of that row of compute_vqa's logits (a wrong row in the second
    # chunk would show here even where two questions have the same answer)
    assert float((ans["logits"][:, 0] - logits.max(dim=1).values).abs().max()) <= 1e-5 and len(set(ans["logits"][:, 0].tolist())) > 200
    assert float((ans3["logits"] - logits.topk(3, dim=1).values).abs().max()) <= 1e-5
    assert ans["answers"] == [[names[i]] for i in preds.tolist()]
    assert bool((ans3["logits"][:, :-1] >= ans3["logits"][:, 1:]).all()) and bool((ans3["scores"] > 0).all())


def test_retrieve_and_recall_on_the_recall_fixture():
    g = load("irtr_recall_L2.npz")
    scores, iids, tiids = torch.from_numpy(g["scores"]).to(DEV), torch.from_numpy(g["iids"]), torch.from_numpy(g["tiids"])
    m = ViLTransformerSS(task_moco(num_layers=1, num_negative=1024, per_gpu_batchsize=2, image_view=True), device=DEV, compute_dtype="f32")
    pr = Predictor(m)
    got = pr.recall(scores, iids, tiids)
    want = objectives.irtr_recall_from_scores(scores, iids, tiids)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and [float(x) for x in got] == [float(np.float32(x)) for x in g["recalls"]]
    r = pr.retrieve(scores, iids, tiids, k=10)
    s = g["scores"]
    cap = np.argsort(-s, axis=1, kind="stable")[:, :10]
    img = np.argsort(-s.T, axis=1, kind="stable")[:, :10]
    assert np.array_equal(r["captions"].cpu().numpy(), cap) and np.array_equal(r["images"].cpu().numpy(), img)
    assert np.array_equal(r["caption_scores"].cpu().numpy(), np.take_along_axis(s, cap, 1))
    assert np.array_equal(r["image_scores"].cpu().numpy(), np.take_along_axis(s.T, img, 1))
    assert np.array_equal(r["caption_iids"].cpu().numpy(), g["tiids"][cap]) and np.array_equal(r["image_iids"].cpu().numpy(), g["iids"][img])
    # exact ties go to the smaller index in both directions
    tie = scores.clone()
    tie[:, 5] = tie[:, 2]
    tie[7] = tie[3]
    rt = pr.retrieve(tie, iids, tiids, k=11)
    assert np.array_equal(rt["captions"].cpu().numpy(), np.argsort(-tie.cpu().numpy(), axis=1, kind="stable")[:, :11])
    assert np.array_equal(rt["images"].cpu().numpy(), np.argsort(-tie.cpu().numpy().T, axis=1, kind="stable")[:, :11])
    # Engine.rows_topk reads the row stride: a column slice of a wider matrix, no copy
    wide = torch.full((11, 24), 9e9, device=DEV)
    wide[:, 3:18] = scores
    idx, val, prob = m.engine.rows_topk(wide[:, 3:18], 4, "sigmoid")
    assert np.array_equal(idx.cpu().numpy(), cap[:, :4]) and torch.equal(val, r["caption_scores"][:, :4])
    assert float((prob - torch.sigmoid(val)).abs().max()) < 1e-6
    _, _, _, lse = m.engine.rows_topk(wide[:, 3:18], 1, "softmax", want_lse=True)
    assert float((lse.double() - torch.logsumexp(scores.double(), 1)).abs().max()) < 1e-5
    for bad in (lambda: m.engine.rows_topk(wide.t(), 2), lambda: m.engine.rows_topk(wide, 25), lambda: m.engine.rows_topk(wide, 33),
                lambda: m.engine.rows_topk(wide.to(torch.bfloat16), 2), lambda: m.engine.rows_topk(wide[None], 2)):
        with pytest.raises(ValueError):
            bad()
    # a model without the heads says so
    batch = {"text_ids": torch.zeros(2, 40, dtype=torch.int64), "text_masks": torch.ones(2, 40, dtype=torch.int64), "image": [torch.zeros(2, 3, 384, 384)]}
    with pytest.raises(ValueError, match=r"loss_names\['mlm'\] > 0"):
        pr.mlm_topk(batch)
    with pytest.raises(ValueError, match=r"loss_names\['mlm'\] > 0"):
        pr.fill_mask(batch["image"][0], text_ids=batch["text_ids"], mask_token_id=103)
    with pytest.raises(ValueError, match=r"loss_names\['vqa'\] > 0"):
        pr.answer(batch)


def test_a_prediction_leaves_no_engine_state_behind():
    """Identical models under dropout: A and A' take one training step, P fills masks, lists candidates and answers first and then takes
    the same step.  The loss has the same bits in all three (the dropout masks are a function of the engine's pass counter, which a
    prediction puts back).  The backward is not bit-reproducible run to run (float atomics of the cls-row scatter: tests/test_resume_gpu.py),
    so the gradient arena is held to that test's rule: P's relative distance from A is at most max(1e-5, 10 * distance(A, A'))."""
    g = load(PO.FIXTURE)
    cfg, p, batch, _ = PO.load_case(g, "equal")
    tb = M.synthetic_mlm(dict(batch, text_ids=torch.from_numpy(g["equal_final_ids"])), 5, cfg["vocab_size"])
    tb["vqa_labels"], tb["vqa_scores"] = V.synthetic_labels(PO.B, 6)
    out = []
    for predict_first in (False, False, True):
        torch.manual_seed(3)
        m = make_module(p, "bf16", drop_rate=0.1)
        m.train()
        if predict_first:
            pr = Predictor(m, tokenizer=PO.VOCAB)
            pr.fill_mask(batch["image"][0], text_ids=batch["text_ids"], text_masks=batch["text_masks"])
            pr.mlm_topk(dev_batch(batch), k=3)
            pr.answer(dev_batch(batch))
            assert m.training and all(mod.training for mod in m.modules())
        m.zero_grad()
        loss = m.training_step(dev_batch(tb), 0)
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.detach().clone(), m.engine.g32.clone()))
    assert torch.isfinite(out[0][0]) and float(out[0][1].abs().max()) > 0
    for other in out[1:]:
        assert torch.equal(out[0][0].view(torch.int32), other[0].view(torch.int32))
    dist = lambda a, b: float((a - b).norm() / a.norm())
    assert dist(out[0][1], out[2][1]) <= max(1e-5, 10 * dist(out[0][1], out[1][1]))
