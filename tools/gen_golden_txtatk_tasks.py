"""Generate tests/golden/txtatk_vqa_L2_B4.npz and txtatk_nlvr2_L2_B4.npz by running the REFERENCE's own GreedyAttack_vqa /
GreedyAttack_nlvr2.adv_attack_samples (attack/greedy_attack_vilt.py:835-1043, :1263-1478) inside its compute_vqa_attack /
compute_nlvr2_attack (vilt/modules/objectives.py:813-859, :898-1000) with text_view=True, alone and together with image_view (K = 2).

TEST INFRASTRUCTURE ONLY: runs on the build machine only (needs the reference checkout that oracle/gen_golden.py imports).  It imports
oracle.gen_golden unchanged (its stand-ins, Holder, tensor_digest, TOY_SENTENCES), wraps the reference's methods to record what they
return and edits nothing in the reference.  Inputs: the toy vocabulary / counter-fitted vectors / stop words already in tests/golden, the
seeded heads and labels of tests/vqa_oracle.py / tests/nlvr2_oracle.py (tests/txtatk_tasks_oracle.py case_inputs).  Adaptations, as in
oracle.gen_golden.run_text_attack_words: the attacker object is made with __new__ and given the attributes __init__ (:48-74) would set
(its __init__ loads resources by name from the network); the installed tokenizer gets the `_convert_token_to_id` the reference calls
(:277); and `Tensor.cuda` is a no-op while the reference runs (GreedyAttack_vqa.get_grad moves its loss with `.cuda(self.device)`, :1324).
Run with PYTHONHASHSEED=0: the reference keeps candidates in Python sets.

NLVR2's train branch of compute_nlvr2_attack reads a key it never sets (objectives.py:944-946), so the NLVR2 objective runs in the val
phase (drop_rate is 0: the arithmetic is the train phase's), like tools/gen_golden_nlvr2.py.

Margin condition.  Discrete decisions can flip under fp32 reordering, so for every decision the fixture records the reference's margin:
`cand_margin` (best minus runner-up candidate loss of every changed sample with more than one candidate) and `word_gap` (relative gap
between the two highest eligible word scores).  The CPU oracle (tests/txtatk_tasks_oracle.py replay) recomputes everything; the largest
|oracle - reference| candidate loss (`oracle_loss_diff`) and relative word-score difference (`oracle_score_rel_diff`) are recorded too,
and the seeds are REFUSED unless min(cand_margin) >= 100 x oracle_loss_diff and min(word_gap) >= 100 x oracle_score_rel_diff, at least two
samples change a word, at least one sample has no eligible word in some loop, and one accepted pick has index 0.

Usage:  PYTHONHASHSEED=0 python tools/gen_golden_txtatk_tasks.py [vqa] [nlvr2]      (~2 min)
"""
from __future__ import annotations

import os
import sys
import tempfile
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins, imports the reference)
from attack.greedy_attack_vilt import GreedyAttack_vqa, GreedyAttack_nlvr2  # noqa: E402  (reference, unmodified)
from attack.pgd_attack_vilt import PGDAttack_vqa, PGDAttack_nlvr2  # noqa: E402  (reference, unmodified)
from tests import golden_util  # noqa: E402
from tests import txtatk_tasks_oracle as T  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SUB = 4                     # the recorded gradients keep every 4th hidden column (file size)


def _tokenizer():
    from transformers import BertTokenizer

    class Tok(BertTokenizer):
        def _convert_token_to_id(self, token):
            return self.convert_tokens_to_ids(token)

    with open(os.path.join(GOLD, "toy_vocab.txt")) as f:
        vocab = {line.rstrip("\n"): i for i, line in enumerate(f)}
    return Tok(vocab=vocab, do_lower_case=True)


def _ref_attacker(cls, name, cfg, tok):
    from torch.nn import CosineSimilarity
    g = cls.__new__(cls)
    g.pl_module, g.contrastive_framework = None, name
    g.stopwords = set(G.TOY_STOP)
    g.cosine_similarity = CosineSimilarity(dim=1, eps=1e-6)
    g.tokenizer = tok
    g.device, g.words_to_sub_words = None, None
    g.max_length, g.n_candidates, g.max_loops, g.sim_thred = cfg["max_text_len"], cfg["n_candidates"], cfg["max_loops"], 0.5
    g.word2id = tok.get_vocab()
    g.id2word = {v: kk for kk, v in g.word2id.items()}
    g.cos_sim = g.sim_word2id = g.sim_id2word = g.cos_sim_dict = None
    g.synonym = "cos_sim"
    g.max_image_len = cfg["max_image_len"]
    g.vqa_classifier = g.nlvr2_classifier = None
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:                       # init_matrix saves its cosine matrix into the cwd (:97)
        os.chdir(tmp)
        try:
            g.init_matrix(os.path.join(GOLD, "toy_counter_fitted.txt"), os.path.join(tmp, "absent.npy"))
        finally:
            os.chdir(cwd)
    return g


def _trace(g):
    """wrap the attacker's methods: what each returns, per loop"""
    tr = {"replace_idx": [], "all_new_text": [], "all_num": [], "best_idx": [], "cand_loss": [], "grads": [], "ids": [], "masks": [],
          "text": [], "scores": []}
    cwi, cns, spf, gg, gis = g.compute_word_importance, g.construct_new_samples, g.split_forward, g.get_grad, g.get_important_scores

    def w_gg(*a, **kw):
        out = gg(*a, **kw)
        tr["grads"].append(np.array(out[1], dtype=np.float32))
        tr["ids"].append(a[0].numpy().copy())
        tr["masks"].append(a[1].numpy().copy())
        tr["text"].append(list(a[2]))
        tr["scores"].append([])
        return out

    def w_gis(*a, **kw):
        out = gis(*a, **kw)
        tr["scores"][-1].append(np.array([float(x) for x in out], dtype=np.float64))
        return out

    def w_cwi(**kw):
        out = cwi(**kw)
        tr["replace_idx"].append([-1 if x is None else int(x) for x in out[0]])
        return out

    def w_cns(**kw):
        out = cns(**kw)
        tr["all_new_text"].append(list(out[0]))
        tr["all_num"].append(list(out[1]))
        return out

    def w_spf(*a, **kw):
        out = spf(*a, **kw)
        tr["best_idx"].append([int(j) for _, j in out])
        tr["cand_loss"].append([float(x) for cl, _ in out for x in cl])
        return out

    g.get_grad, g.get_important_scores, g.compute_word_importance, g.construct_new_samples, g.split_forward = w_gg, w_gis, w_cwi, w_cns, w_spf
    return tr


def _score(logits, targets):
    idx = torch.max(logits.detach().float(), 1)[1]
    one_hots = torch.zeros(*targets.size()).to(targets)
    one_hots.scatter_(1, idx.view(-1, 1), 1)
    return (one_hots * targets).sum() / len(idx)


def _holder(task, cfg, p):
    h = G.Holder(cfg)
    D = cfg["hidden_size"]
    if task == "vqa":
        h.vqa_classifier = nn.Sequential(nn.Linear(D, 2 * D), nn.LayerNorm(2 * D), nn.GELU(), nn.Linear(2 * D, cfg["vqav2_label_size"]))
        h.pgd_attacker = PGDAttack_vqa(cfg)
        for phase in ("train", "val"):
            setattr(h, f"{phase}_vqa_attacked_loss", lambda x: x)
            setattr(h, f"{phase}_vqa_attacked_score", _score)
    else:
        h.nlvr2_classifier = nn.Sequential(nn.Linear(2 * D, 2 * D), nn.LayerNorm(2 * D), nn.GELU(), nn.Linear(2 * D, 2))
        h.token_type_embeddings = nn.Embedding(3, D)
        h.attack_idx = [True, True]
        h.pgd_attacker = PGDAttack_nlvr2(dict(cfg, attack_idx=h.attack_idx))
        acc = lambda lg, lb: (lg.argmax(-1) == lb).float().mean()
        chg = lambda la, lo: (la.argmax(-1) != lo.argmax(-1)).float().mean()
        for ph in ("train", "dev", "test"):
            for t in ("nlvr2", "nlvr2_original", "nlvr2_attacked"):
                setattr(h, f"{ph}_{t}_loss", lambda x: x)
                setattr(h, f"{ph}_{t}_accuracy", acc)
            setattr(h, f"{ph}_nlvr2_attacked_change_rate_cross", chg)
    h.load_oracle_params({n: t for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))})
    return h


def _objective(task, cfg, p, batch, tok, both):
    """one run of the reference's compute_{vqa,nlvr2}_attack with text_view (and image_view when `both`): (outputs, attack trace, result)"""
    torch.manual_seed(888)
    h = _holder(task, cfg, p)
    h.text_view, h.image_view = True, bool(both)
    g = _ref_attacker(GreedyAttack_vqa if task == "vqa" else GreedyAttack_nlvr2, task, cfg, tok)
    h.greedy_attacker = g
    tr = _trace(g)
    res = {}
    aas = g.adv_attack_samples

    def w_aas(*a, **kw):
        out = aas(*a, **kw)
        res.update(out)
        return out

    g.adv_attack_samples = w_aas
    params = [(n, prm) for n, prm in h.named_parameters() if not n.startswith("k_")]
    attack = h.pgd_attacker.pgd_attack

    def recording_attack(pl_module, b_, **kw):
        d = attack(pl_module, b_, **kw)
        for n, prm in params:                       # PGDAttack_vqa back-propagates through the live module: the leaked weight gradients
            prm.grad = None                         # are not stepped (INTEGRATION.md "VQA"); PGDAttack_nlvr2 attacks a deep copy
        return d

    h.pgd_attacker.pgd_attack = recording_attack
    h.zero_grad()
    if task == "vqa":
        h.train()
        ret = G.objectives.compute_vqa_attack(h, deepcopy(batch))
        total = ret["vqa_loss"]
    else:
        h.eval()
        ret = G.objectives.compute_nlvr2_attack(h, deepcopy(batch))
        total = ret["nlvr2_original_loss"] + ret["nlvr2_attacked_loss"]
    total.backward()
    out = {"total_loss": np.float64(total.item())}
    for k, v in ret.items():
        if k.endswith("_loss"):
            out[k] = np.float64(v.item())
        elif k.endswith("_logits"):
            out[k] = v.detach().numpy()
    for kk, v in h.logged.items():
        out["log_" + kk.replace("/", "__")] = np.float64(v)
    gnames, gd = [], []
    for n, prm in params:
        if prm.grad is not None:
            gnames.append(n)
            gd.append(G.tensor_digest(prm.grad))
    out["grad_names"] = np.array(gnames)
    out["grad_digest"] = np.stack(gd)
    return out, tr, res, g


def run(task):
    B, sw, sh, sb, sl, layers, loops, ncand, K = T.CASES[task]
    sentences = G.TOY_SENTENCES[:B]
    cfg, p, batch = T.case_inputs(task, sentences)
    tok = _tokenizer()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        o_txt, tr, res, g = _objective(task, cfg, p, batch, tok, both=False)
        o_both, tr2, res2, _ = _objective(task, cfg, p, batch, tok, both=True)
    finally:
        torch.Tensor.cuda = cuda
    # with both views the text attack runs on a deepcopy of the CLEAN batch: the same attack
    assert res2["text"] == res["text"] and tr2["best_idx"] == tr["best_idx"] and tr2["replace_idx"] == tr["replace_idx"]
    for c1, c2 in zip(tr["cand_loss"], tr2["cand_loss"]):            # (two runs of the reference differ by an fp32 ulp of the loss)
        np.testing.assert_allclose(c1, c2, rtol=1e-6)
    words = sorted(g.sim_word2id, key=g.sim_word2id.get)
    out = {
        "text_in": np.array(sentences), "text_ids_in": batch["text_ids"].numpy(), "text_masks_in": batch["text_masks"].numpy(),
        "text_out": np.array(res["text"]), "text_ids_out": res["txt_input_ids"].numpy(), "text_masks_out": res["text_masks"].numpy(),
        "num_changes": np.float64(res["num_changes"]), "change_rate": np.float64(res["change_rate"]),
        "problem": np.array(bool(res["Problem"])), "changes_verification": np.array(res["changes_verification"]),
        "replace_idx": np.array(tr["replace_idx"]), "best_idx": np.array(tr["best_idx"]),
        "ids_loops": np.stack(tr["ids"]), "masks_loops": np.stack(tr["masks"]),
        "grads_loop0_sub": tr["grads"][0][:, :, ::SUB].copy(),
        "syn_words": np.array(words),
        # the reference's candidate sets in ITS iteration order (a set: depends on the hash seed), '|'-joined per word
        "syn_cands": np.array(["|".join(g.cos_sim_dict[g.sim_word2id[w]]) for w in words]),
        "meta": np.array([B, sw, sh, sb, sl, layers, loops, ncand, K]),
    }
    for li in range(loops):
        out[f"text_{li}"] = np.array(tr["text"][li])
        out[f"new_text_{li}"] = np.array(tr["all_new_text"][li])
        out[f"all_num_{li}"] = np.array(tr["all_num"][li])
        out[f"cand_loss_{li}"] = np.array(tr["cand_loss"][li])
        for b in range(B):
            out[f"scores_{li}_{b}"] = tr["scores"][li][b]
    for view, o in (("txt", o_txt), ("both", o_both)):
        for k, v in o.items():
            out[f"{view}_{k}"] = v
    # ---- the CPU oracle on the recorded run: differences, margins, which pass's embedding gradient ----------------------------------
    rp = T.replay(task, out)
    assert rp["replace_idx"] == out["replace_idx"].tolist(), (rp["replace_idx"], out["replace_idx"].tolist())
    assert rp["picks"] == out["best_idx"].tolist(), (rp["picks"], out["best_idx"].tolist())
    assert rp["changes_verification"] == out["changes_verification"].tolist()
    g0 = tr["grads"][0]
    pass_diff = [float(np.abs(g0 - x).max()) for x in rp["grads_loop0"]]
    out["emb_grad_pass_diff"] = np.array(pass_diff)                   # max |grads - oracle gradient of pass i|: i = 0 (image_0), 1 (image_1)
    for i, x in enumerate(rp["grads_loop0"]):
        out[f"oracle_grads_pass{i}_sub"] = x[:, :, ::SUB].copy()
    out["grads_absmax"] = np.float64(np.abs(g0).max())
    out["oracle_loss_diff"] = np.float64(rp["loss_diff"])
    out["oracle_score_rel_diff"] = np.float64(rp["score_rel_diff"])
    out["cand_margin"] = np.array(rp["cand_margin"])
    out["word_gap"] = np.array(rp["word_gap"])
    print(task, "final", res["text"], "changes", res["changes_verification"], "replace", tr["replace_idx"], "picks", tr["best_idx"])
    print(task, "pass diff", pass_diff, "|g|max", out["grads_absmax"], "loss diff", rp["loss_diff"], "score rel diff", rp["score_rel_diff"],
          "min cand margin", min(rp["cand_margin"]), "min word gap", min(rp["word_gap"]))
    assert pass_diff[-1] < 1e-3 * float(out["grads_absmax"]), "the recorded saliency is not the LAST pass's embedding gradient"
    assert min(rp["cand_margin"]) >= T.MARGIN_FACTOR * rp["loss_diff"], "seed refused: candidate margin"
    assert min(rp["word_gap"]) >= T.MARGIN_FACTOR * rp["score_rel_diff"], "seed refused: word score gap"
    assert sum(1 for c in res["changes_verification"] if c > 0) >= 2, "seed refused: fewer than two samples change a word"
    assert any(x == -1 for row in tr["replace_idx"] for x in row), "seed refused: no sample without an eligible word"
    assert any(j == 0 and r >= 0 for rr, bb in zip(tr["replace_idx"], tr["best_idx"]) for r, j in zip(rr, bb)), "seed refused: no pick 0"
    path = os.path.join(GOLD, T.FIXTURE[task])
    golden_util.save(path, out)
    print(os.path.basename(path), os.path.getsize(path), "bytes", {k: float(v) for k, v in out.items() if k.endswith("_loss")},
          {k: float(v) for k, v in out.items() if "log_" in k})


if __name__ == "__main__":
    torch.set_num_threads(8)
    for task in (sys.argv[1:] or ["vqa", "nlvr2"]):
        run(task)
