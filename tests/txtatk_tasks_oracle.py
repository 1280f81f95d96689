"""CPU oracle of the text view of the attacked VQA / NLVR2 tasks (test infrastructure): the tensor side of the reference's
GreedyAttack_vqa / GreedyAttack_nlvr2 (attack/greedy_attack_vilt.py:835-1043, :1263-1478) restated in torch on oracle.rmcl_oracle and the
heads of tests/vqa_oracle.py / tests/nlvr2_oracle.py, the seeded inputs tools/gen_golden_txtatk_tasks.py feeds the reference, and a
replay that recomputes every recorded decision and loss of a txtatk_{vqa,nlvr2}_* fixture from (cfg, seeds, sentences) alone.

The linguistic host side (word <-> sub-word map, word filter, synonym membership) is the product's attack/word_substitution.py, which the
CPU suite already pins against the reference (tests/test_oracle_golden.py).

Arithmetic restated here:
* saliency = gradient of the batch loss at the OUTPUT of word_embeddings; NLVR2 calls word_embeddings twice (infer1: image_0 / token type
  1, infer2: image_1 / token type 2) and the reference reads emb_grads[0] only (:894) - both per-pass gradients are formed so that a
  fixture can say which one that is;
* word score = L1 norm of the mean gradient over a word's sub-word tokens (:221-228);
* candidate j of sample i is scored by the batch loss with row i replaced; `t_save = ori_z[i]` (:912, :1343) is a view, so the restore is a
  no-op and row r < i keeps its LAST candidate: loss_ij = (sum_b s_b + sum_{r<i} (c_{r,last} - s_r) + c_ij - s_i) / B on per-row terms;
* the running maximum starts at -1, the first strict maximum wins, a changed sample takes it when its loss is > 0 (:1010, :1445)."""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rmcl_oracle as O
from tests import nlvr2_oracle as N
from tests import vqa_oracle as V

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN_FACTOR = 100.0        # every recorded decision margin is at least this many times the oracle-vs-reference difference

# task -> (B, seed_w, seed_h, seed_b, seed_l, layers, max_loops, n_candidates, K of the both-views step)
CASES = {"vqa": (4, 11, 55, 24, 65, 2, 3, 5, 2), "nlvr2": (4, 13, 75, 35, 0, 2, 3, 5, 2)}
# The reference scores a VQA candidate by the fp32 value of the WHOLE batch loss.  At vqav2_label_size = 3129 that value is ~2 200 (3129 x
# softplus(~0)), one fp32 ulp of it is 2.4e-4, and a synonym moves it by 1e-3: two runs of the reference itself differ by an ulp, and no
# seed comes near the margin condition (best minus runner-up >= 100 x the oracle's difference).  The fixture therefore uses a 16-answer
# head (loss ~14, ulp 1e-6) whose output layer - vqa_oracle's seeded N(0, 0.02) weights - is scaled by 4 (logits of std ~2 instead of
# ~0.5), which lifts the smallest decision margin to ~250 ulps.  The 3129-answer head is covered by tests/test_vqa_gpu.py, the 257-row chunk
# test and tests/test_txtatk_tasks_gpu.py::test_vqa_attack_runs_on_the_3129_answer_head (runs, finite, device and host scores agree).
VQA_LABELS = 16
VQA_GAIN = 4.0
FIXTURE = {"vqa": "txtatk_vqa_L2_B4.npz", "nlvr2": "txtatk_nlvr2_L2_B4.npz"}


def toy_resources(n_candidates: int):
    """(tokenizer, synonym table, word filter) from the toy vocabulary / counter-fitted vectors / stop words of tests/golden"""
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.attack import word_substitution as WS
    tok = WS.load_tokenizer(os.path.join(GOLD, "toy_vocab.txt"))
    table = WS.SynonymTable(os.path.join(GOLD, "toy_counter_fitted.txt"), n_candidates=n_candidates, sim_thred=0.5)
    return tok, table, WS.WordFilter(WS.load_stopwords(os.path.join(GOLD, "toy_stopwords.txt")))


def case_inputs(task: str, sentences: List[str]):
    """(cfg, params incl. the task head, batch with the tokenised `sentences`) of a fixture, from its seeds alone"""
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.attack import word_substitution as WS
    B, sw, sh, sb, sl, layers, loops, ncand, K = CASES[task]
    cfg = O.default_config(num_layers=layers, num_negative=1024, adv_steps_img=K, per_gpu_batchsize=B, max_loops=loops, n_candidates=ncand,
                           vqav2_label_size=VQA_LABELS)
    p = O.init_params(cfg, sw)
    if task == "vqa":
        p.update(V.vqa_init_params(cfg, sh))
        p["vqa_classifier.3.weight"] = p["vqa_classifier.3.weight"] * VQA_GAIN
        batch = O.synthetic_batch(cfg, B, sb)
        batch["vqa_labels"], batch["vqa_scores"] = V.synthetic_labels(B, sl, VQA_LABELS)
    else:
        p.update(N.nlvr2_init_params(cfg, p, sh))
        batch = N.synthetic_pairs(cfg, B, sb)
    tok = WS.load_tokenizer(os.path.join(GOLD, "toy_vocab.txt"))
    ids, masks = WS.encode_sentences(tok, list(sentences), cfg["max_text_len"])
    batch["text"], batch["text_ids"], batch["text_masks"] = list(sentences), ids, masks
    return cfg, p, batch


# ---- tensor side ---------------------------------------------------------------------------------------------------------------------
def _rows_vqa(p, logits, targets):
    return F.binary_cross_entropy_with_logits(logits, targets, reduction="none").sum(dim=1)


def rows(task, p, cfg, batch, ids, masks, owner=None, want_grad=False):
    """Per-row loss terms (VQA: BCE row sums; NLVR2: row CE) of the sentences (ids, masks), sentence r with the images / labels of sample
    owner[r] (None: r).  want_grad: also the gradients of the batch loss (mean of the rows) at the word_embeddings output - VQA: [g];
    NLVR2: [g of the image_0 / type-1 pass, g of the image_1 / type-2 pass]."""
    own = torch.arange(ids.shape[0]) if owner is None else torch.as_tensor(owner)
    W = p["text_embeddings.word_embeddings.weight"].detach()
    n_we = 1 if task == "vqa" else 2
    wes = [W[ids].clone().requires_grad_(want_grad) for _ in range(n_we)]
    with torch.set_grad_enabled(want_grad):
        if task == "vqa":
            cls = O.infer(p, cfg, ids, masks, batch["image"][0][own], word_embeds=wes[0])["cls_feats"]
            targets = V.dense_targets(batch["vqa_labels"], batch["vqa_scores"], len(batch["vqa_labels"]), cfg["vqav2_label_size"])[own]
            r = _rows_vqa(p, V.vqa_head(p, cls), targets)
        else:
            c1 = O.infer(p, cfg, ids, masks, batch["image_0"][0][own], image_token_type_idx=1, word_embeds=wes[0])["cls_feats"]
            c2 = O.infer(p, cfg, ids, masks, batch["image_1"][0][own], image_token_type_idx=2, word_embeds=wes[1])["cls_feats"]
            r = F.cross_entropy(N.nlvr2_head(p, torch.cat([c1, c2], dim=-1)), N.labels_of(batch)[own], reduction="none")
        if not want_grad:
            return r.detach()
        grads = torch.autograd.grad(r.mean(), wes)
    return r.detach(), [g.detach() for g in grads]


def word_scores(grads_b: np.ndarray, mapping: Dict[int, np.ndarray]) -> List[float]:
    """get_important_scores (:221-228) on grads_b = the rows of one sentence WITHOUT its [CLS] row"""
    return [float(np.abs(grads_b[mapping[i]].astype(np.float64).mean(axis=0)).sum()) for i in range(len(mapping))]


def eligible(words, history, spent: bool, check_word, known) -> List[int]:
    """word indices compute_word_importance (:290-301) may pick"""
    if spent:
        return []
    out = []
    for i, w in enumerate(words):
        w = w.strip().lower()
        if check_word(w) or w not in known or i in history:
            continue
        out.append(i)
    return out


def select(s, c, all_num, B):
    """split_forward (:900-931, :1333-1369) on per-row terms: [(losses, pick)] per sample"""
    tot, drift, r0, out = float(sum(s)), 0.0, 0, []
    for i in range(B):
        best, pick, losses = -1.0, -1, []
        for j in range(all_num[i]):
            lj = (tot + drift + c[r0 + j] - s[i]) / B
            losses.append(lj)
            if lj > best:
                best, pick = lj, j
        drift += c[r0 + all_num[i] - 1] - s[i]
        r0 += all_num[i]
        out.append((losses, pick))
    return out


def replay(task: str, g) -> dict:
    """Recomputes a fixture loop by loop from the sentences it recorded for that loop: the word attacked, the candidate losses (for the
    fixture's candidate sentences, in its order), the picks.  Returns the recomputed values, the largest differences to the recorded ones, and the
    decision margins of the RECORDED values: per changed sample with more than one candidate the gap between the best and the runner-up
    candidate loss, per word decision the relative gap between the two highest eligible word scores (1.0 when only one is eligible)."""
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.attack import word_substitution as WS
    B, sw, sh, sb, sl, layers, loops, ncand, K = CASES[task]
    cfg, p, batch = case_inputs(task, [str(t) for t in g["text_in"]])
    tok, table, check_word = toy_resources(ncand)
    Lt = cfg["max_text_len"]
    history = [set() for _ in range(B)]
    changes = [0] * B
    out = {"replace_idx": [], "picks": [], "losses": [], "loss_diff": 0.0, "score_rel_diff": 0.0, "cand_margin": [], "word_gap": [],
           "grads_loop0": None}
    for li in range(loops):
        text = [str(t) for t in g[f"text_{li}"]]
        ids, masks = WS.encode_sentences(tok, text, Lt)
        # loop 0: the words are the DECODED ids (:946-948: "dogs" is the two words "dog" and "##s"); later loops: the chosen sentences
        words = [WS.decode_words(tok, ids[b_]) for b_ in range(B)] if li == 0 else [t.split(" ") for t in text]
        assert np.array_equal(ids.numpy(), g["ids_loops"][li])
        s, grads = rows(task, p, cfg, batch, ids, masks, want_grad=True)
        gsal = grads[-1].numpy()                                        # NLVR2: the image_1 / token-type-2 pass (emb_grads[0])
        if li == 0:
            out["grads_loop0"] = [x.numpy() for x in grads]
        sep = [int((ids[b] == 102).nonzero()[0]) for b in range(B)]
        ridx = []
        for b in range(B):
            mapping = WS.words_to_sub_words(tok, words[b], Lt)
            sc = word_scores(gsal[b][1:], mapping)
            ref_sc = g[f"scores_{li}_{b}"]
            out["score_rel_diff"] = max(out["score_rel_diff"], float(np.max(np.abs(np.array(sc) - ref_sc) / np.abs(ref_sc))))
            el = [i for i in eligible(words[b], history[b], changes[b] >= min(int(sep[b] * 0.2), loops), check_word, table) if i < len(sc)]
            if not el:
                ridx.append(-1)
                continue
            order = sorted(el, key=lambda i: -sc[i])
            ridx.append(order[0])
            history[b].add(order[0])
            rs = sorted((float(ref_sc[i]) for i in el), reverse=True)            # the margin is the REFERENCE's own
            out["word_gap"].append(1.0 if len(rs) == 1 else (rs[0] - rs[1]) / rs[0])
        out["replace_idx"].append(ridx)
        new_text = [str(t) for t in g[f"new_text_{li}"]]
        all_num = [int(x) for x in g[f"all_num_{li}"]]
        owner = [b for b in range(B) for _ in range(all_num[b])]
        cids, cmasks = WS.encode_sentences(tok, new_text, Lt)
        c = rows(task, p, cfg, batch, cids, cmasks, owner=owner)
        picks = select(s.double().tolist(), c.double().tolist(), all_num, B)
        flat = [x for ls, _ in picks for x in ls]
        out["losses"].append(flat)
        out["loss_diff"] = max(out["loss_diff"], float(np.max(np.abs(np.array(flat) - g[f"cand_loss_{li}"]))))
        out["picks"].append([j for _, j in picks])
        r0 = 0
        for b, (ls, j) in enumerate(picks):
            if ridx[b] >= 0:
                if len(ls) > 1:
                    top = sorted((float(x) for x in g[f"cand_loss_{li}"][r0:r0 + len(ls)]), reverse=True)   # the REFERENCE's own margin
                    out["cand_margin"].append(top[0] - top[1])
                if ls[j] > 0:
                    changes[b] += 1
            r0 += len(ls)
    out["changes_verification"] = changes
    return out
