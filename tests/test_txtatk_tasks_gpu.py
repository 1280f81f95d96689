"""-m gpu: the text view of task_finetune_vqa_randaug_attacked / task_finetune_nlvr2_randaug_attacked (GreedyAttack_vqa /
GreedyAttack_nlvr2, alone and with the image view) against the reference's own run on the toy vocabulary
(tests/golden/txtatk_{vqa,nlvr2}_L2_B4.npz from tools/gen_golden_txtatk_tasks.py): every word attacked, candidate sentence, candidate loss
and pick per loop, the final sentences / ids / masks / statistics, and the objectives' losses, logits, logs and gradient digests.
Candidates are fed in the reference's recorded iteration order (it keeps them in a Python set), as in
tests/test_parity2_gpu.py::test_word_level_text_attack_matches_reference_end_to_end."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd.vilt.config import task_finetune_vqa_randaug_attacked, task_finetune_nlvr2_randaug_attacked  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, vilt_utils  # noqa: E402
from tests import txtatk_tasks_oracle as T  # noqa: E402
from tests.golden_util import digest, load  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"
# the f32 tolerances of tests/test_vqa_gpu.py and tests/test_nlvr2_gpu.py (the repository's fp32 contract)
TOL = dict(loss=1e-3, logits=2e-3, grad=2e-3, delta=5e-5)
_CASES = {}


def _case(task):
    """(fixture, oracle cfg, params, host batch), loaded once per task"""
    if task not in _CASES:
        g = load(T.FIXTURE[task])
        _CASES[task] = (g,) + T.case_inputs(task, [str(t) for t in g["text_in"]])
    return _CASES[task]


def make_module(task, dtype="f32", both=False, ref_order=True, **over):
    g, cfg, p, _ = _case(task)
    kw = dict(num_layers=cfg["num_layers"], per_gpu_batchsize=cfg["per_gpu_batchsize"], adv_steps_img=cfg["adv_steps_img"], drop_rate=0.0,
              max_steps=100, warmup_steps=0, text_view=True, image_view=both, max_loops=cfg["max_loops"], n_candidates=cfg["n_candidates"],
              tokenizer=os.path.join(T.GOLD, "toy_vocab.txt"), embedding_path=os.path.join(T.GOLD, "toy_counter_fitted.txt"),
              stopwords=os.path.join(T.GOLD, "toy_stopwords.txt"))
    kw.update(over)
    if task == "vqa":
        c = task_finetune_vqa_randaug_attacked(vqav2_label_size=T.VQA_LABELS, **kw)
    else:
        c = task_finetune_nlvr2_randaug_attacked(attack_idx=[True, True], **kw)
    m = ViLTransformerSS(c, device=DEV, compute_dtype=dtype)
    sd = {n: t.to(DEV) for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    if ref_order:
        table = m.greedy_attacker.synonyms
        order = {str(w): str(c_).split("|") for w, c_ in zip(g["syn_words"], g["syn_cands"])}

        class RefOrder:
            word2id = table.word2id
            __contains__ = lambda self, w: w in table.word2id
            __call__ = lambda self, w: order.get(w, [w])

        m.greedy_attacker.synonyms = RefOrder()
    m.train()
    return m


def _run(m, batch, train=True):
    """forward of the module's tasks; train: also the backward of every loss key (what training_step sums)"""
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


def _snapshot(batch):
    return {k: ([t.clone() for t in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else (v.clone() if torch.is_tensor(v) else
                                                                                                   list(v) if isinstance(v, list) else v))
            for k, v in batch.items()}


def _assert_unchanged(batch, snap):
    assert batch.keys() == snap.keys()
    for k, v in snap.items():
        if isinstance(v, list) and v and torch.is_tensor(v[0]):
            assert all(torch.equal(a, b) for a, b in zip(batch[k], v)), k
        elif torch.is_tensor(v):
            assert torch.equal(batch[k], v), k
        else:
            assert batch[k] == v, k


@pytest.mark.parametrize("task", ["vqa", "nlvr2"])
def test_attack_matches_reference_end_to_end(task):
    g, cfg, p, batch = _case(task)
    m = make_module(task)
    db = dev_batch(batch)
    snap = _snapshot(db)
    att = m.greedy_attacker
    res = att.adv_attack_samples(m, db, None)
    assert len(att.trace) == cfg["max_loops"]
    for li, (replace_idx, new_text, all_num, best) in enumerate(att.trace):
        assert [-1 if x is None else x for x in replace_idx] == g["replace_idx"][li].tolist(), li          # the words attacked
        assert new_text == [str(t) for t in g[f"new_text_{li}"]] and all_num == g[f"all_num_{li}"].tolist(), li
        ref = g[f"cand_loss_{li}"]
        print(task, "loop", li, "max |candidate loss - reference|", float(np.abs(np.array(att.loss_trace[li]) - ref).max()))
        np.testing.assert_allclose(att.loss_trace[li], ref, rtol=TOL["loss"], atol=0)
        assert best == g["best_idx"][li].tolist(), li                                                          # the picks, index 0 included
    assert res["text"] == [str(t) for t in g["text_out"]]
    assert torch.equal(res["txt_input_ids"].cpu(), torch.from_numpy(g["text_ids_out"]))
    assert torch.equal(res["text_masks"].cpu(), torch.from_numpy(g["text_masks_out"]))
    assert res["changes_verification"] == g["changes_verification"].tolist()
    assert abs(res["num_changes"] - float(g["num_changes"])) < 1e-12 and abs(res["change_rate"] - float(g["change_rate"])) < 1e-12
    assert bool(res["Problem"]) == bool(g["problem"])
    _assert_unchanged(db, snap)
    # the device word scores are the host path's: same decisions with the kernel switched off
    att.device_scores = False
    res_h = att.adv_attack_samples(m, db, None)
    assert res_h["text"] == res["text"] and [[-1 if x is None else x for x in t[0]] for t in att.trace] == g["replace_idx"].tolist()


def _check_grads(m, g, view):
    params = dict(m.named_parameters())
    for n, d in zip(g[f"{view}_grad_names"], g[f"{view}_grad_digest"]):
        got = digest(params[str(n)].grad)
        assert abs(got[1] - d[1]) <= TOL["grad"] * d[1] + 1e-7, (view, str(n), got[:3], d[:3])


@pytest.mark.parametrize("view", ["txt", "both"])
def test_vqa_training_step_matches_reference(view):
    g, cfg, p, batch = _case("vqa")
    m = make_module("vqa", both=view == "both")
    db = dev_batch(batch)
    snap = _snapshot(db)
    m.zero_grad()
    loss = m.training_step(db, 0)
    loss.backward()
    torch.cuda.synchronize()
    ref = float(g[f"{view}_vqa_loss"])
    assert abs(float(loss) - ref) < TOL["loss"] * ref
    assert abs(float(m.logged["vqa_attacked/train/loss"]) - float(g[f"{view}_log_vqa_attacked__train__loss"])) < TOL["loss"] * ref
    assert abs(float(m.logged["vqa_attacked/train/score"]) - float(g[f"{view}_log_vqa_attacked__train__score"])) < 1e-6
    for name in ("num_changes", "change_rate"):                                 # compute_geometric's logs, under the task's name
        assert abs(float(m.logged[f"vqa_attacked_attack/train/{name}"]) - float(g[f"{view}_log_vqa_attacked_attack__train__{name}"])) < 1e-12
    if view == "both":
        assert abs(float(m.logged["vqa_attacked_attack/train/delta"]) - float(g["both_log_vqa_attacked_attack__train__delta"])) < 1e-5
    else:
        assert "vqa_attacked_attack/train/delta" not in m.logged
    lg = m.engine.vqa_bufs(cfg["per_gpu_batchsize"], "vqa_att").logits.cpu().numpy()
    rl = g[f"{view}_vqa_logits"]
    np.testing.assert_allclose(lg, rl, atol=TOL["logits"] * max(1.0, float(np.abs(rl).max())))
    _check_grads(m, g, view)
    _assert_unchanged(db, snap)


@pytest.mark.parametrize("view", ["txt", "both"])
def test_nlvr2_step_and_validation_match_reference(view):
    g, cfg, p, batch = _case("nlvr2")
    m = make_module("nlvr2", both=view == "both")
    db = dev_batch(batch)
    snap = _snapshot(db)
    ret = _run(m, db)
    for k in ("nlvr2_original_loss", "nlvr2_attacked_loss"):
        ref = float(g[f"{view}_{k}"])
        assert abs(float(ret[k]) - ref) < TOL["loss"] * ref, (k, float(ret[k]), ref)
        lk = k.replace("_loss", "_logits")
        rl = g[f"{view}_{lk}"]
        np.testing.assert_allclose(ret[lk].cpu().numpy(), rl, atol=TOL["logits"] * max(1.0, float(np.abs(rl).max())), err_msg=lk)
    assert abs(float(m.logged["nlvr2_attacked/train/loss"]) - float(g[f"{view}_nlvr2_attacked_loss"])) < TOL["loss"] * float(g[f"{view}_nlvr2_attacked_loss"])
    for name in ("num_changes", "change_rate"):
        assert abs(float(m.logged[f"nlvr2_attacked_attack/train/{name}"]) - float(g[f"{view}_log_nlvr2_attacked_attack__val__{name}"])) < 1e-12
    _check_grads(m, g, view)                                                    # of nlvr2_original_loss + nlvr2_attacked_loss
    _assert_unchanged(db, snap)
    # validation phase: every value the reference logged (dev / test rows, change_rate_cross, delta, the attack's statistics)
    m.logged = {}
    _run(m, db, train=False)
    keys = [k for k in g.files if k.startswith(f"{view}_log_")]
    assert any("change_rate_cross" in k for k in keys)
    for k in keys:
        name = k[len(view) + 5:].replace("__", "/")
        if "accuracy" in k or "change_rate_cross" in k:
            atol = 1e-6
        elif "num_changes" in k or "_attack__val__change_rate" in k:
            atol = 1e-12
        elif "loss" in k:
            atol = TOL["loss"] * 2 * float(g[k])
        else:
            atol = TOL["delta"] * 0.2                                           # delta
        assert abs(float(m.logged[name]) - float(g[k])) <= atol, (name, float(m.logged[name]), float(g[k]))
    _assert_unchanged(db, snap)


def test_nlvr2_pair_form_and_two_pass_form_agree():
    g, cfg, p, batch = _case("nlvr2")
    db = dev_batch(batch)
    out = []
    for pair in (True, False):
        m = make_module("nlvr2", nlvr2_pair_pass=pair)
        res = m.greedy_attacker.adv_attack_samples(m, db, None)
        out.append((res, list(m.greedy_attacker.trace), list(m.greedy_attacker.loss_trace)))
    (r1, t1, l1), (r2, t2, l2) = out
    assert r1["text"] == r2["text"] and t1 == t2 and torch.equal(r1["txt_input_ids"], r2["txt_input_ids"])
    for a, b in zip(l1, l2):
        np.testing.assert_allclose(a, b, rtol=1e-6)                             # fp32 summation order only


@pytest.mark.parametrize("task", ["vqa", "nlvr2"])
def test_bf16_step_runs_and_changes_words(task):
    g, cfg, p, batch = _case(task)
    m = make_module(task, dtype="bf16", both=True, ref_order=False)
    db = dev_batch(batch)
    ret = _run(m, db)
    for k, v in ret.items():
        if "loss" in k:
            assert torch.isfinite(v).all(), k
    assert float(m.logged[f"{task}_attacked_attack/train/num_changes"]) * cfg["per_gpu_batchsize"] >= 1
    assert all(torch.isfinite(q.grad).all() for q in m.parameters() if q.grad is not None)


def test_vqa_attack_runs_on_the_3129_answer_head():
    """The fixtures use a 16-answer head (tests/txtatk_tasks_oracle.py says why); this is the real vqav2_label_size = 3129 head with the
    seeded weights of tests/vqa_oracle.py: the attack runs, every candidate loss is finite and positive, words change, and the device
    and the host word-score paths pick the same words in loop 0, where both see the same sentences.  (Later loops are not compared:
    at 3129 answers candidate losses differ by a few fp32 ulps of the batch loss, so a pick - and with it the next loop's sentences -
    may differ between any two runs.)"""
    from tests import vqa_oracle as V
    g, cfg, p, batch = _case("vqa")
    c = dict(cfg, vqav2_label_size=V.N_LABELS)
    p2 = {n: t for n, t in p.items() if not n.startswith("vqa_classifier.")}
    p2.update(V.vqa_init_params(c, 55))
    kw = dict(num_layers=c["num_layers"], per_gpu_batchsize=c["per_gpu_batchsize"], drop_rate=0.0, max_steps=100, warmup_steps=0, text_view=True,
              max_loops=c["max_loops"], n_candidates=c["n_candidates"], tokenizer=os.path.join(T.GOLD, "toy_vocab.txt"),
              embedding_path=os.path.join(T.GOLD, "toy_counter_fitted.txt"), stopwords=os.path.join(T.GOLD, "toy_stopwords.txt"))
    m = ViLTransformerSS(task_finetune_vqa_randaug_attacked(**kw), device=DEV, compute_dtype="f32")
    missing, unexpected = m.load_state_dict({n: t.to(DEV) for n, t in p2.items() if not n.startswith(("k_", "moco_head", "itm_score"))}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    m.train()
    db = dev_batch(batch)
    db["vqa_labels"], db["vqa_scores"] = V.synthetic_labels(c["per_gpu_batchsize"], 65)
    att = m.greedy_attacker
    res = att.adv_attack_samples(m, db, None)
    first = att.trace[0][0]
    assert all(np.isfinite(x) and x > 0 for loop in att.loss_trace for x in loop) and res["num_changes"] > 0
    att.device_scores = False
    att.adv_attack_samples(m, db, None)
    assert att.trace[0][0] == first and any(x is not None for x in first)
