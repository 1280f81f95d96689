"""CPU side of the prediction fixture tests/golden/predict_L2.npz (test infrastructure): the seeded batch on the toy vocabulary, the heads
the fixture describes, the mask-filling loop restated on ids, and the margins of its decisions.  tools/gen_golden_predict.py runs the
loop on the reference's own model and MLMHead and records every decision; tests/test_predict_cpu.py runs it on oracle.rmcl_oracle +
tests/mlm_oracle.py and compares decision by decision; tests/test_predict_gpu.py asks the same of ``rmcl_amd.Predictor``.

Why the heads are designed.  With the seeded N(0, 0.02) heads of tests/mlm_oracle.py / tests/vqa_oracle.py the ranks behind the first are
decided by gaps of a few hundredths of a logit, far below the bf16 logits tolerance of tests/test_mlm_gpu.py (0.1 * max(1, |z|max)) - a
test of the top-5 order or of "the most confident position" would have to skip most of its decisions.  So eight vocabulary rows of
mlm_score.decoder are solved - minimum-norm least squares on the head's input at exactly the positions the loop visits - such that every
visited row has a prescribed ladder: first place at TOP, the runner-up 3 STEP (a "certain" position) or 1 STEP (the "uncertain" one)
below, places 3 to 5 one STEP apart, every other token near FLOOR.  Each position ranks the eight tokens in its own seeded order.

Which position goes first.  The demo compares fp32 softmax probabilities, and in fp32 a probability is exactly 1.0 once the log-odds of
the best token pass SATURATION = 25 ln 2 = 17.33.  Four positions whose probabilities differ by twice the bf16 tolerance each
(2 * 0.1 * 36 = 7.2 logits of log-odds) would need log-odds up to 29: the upper ones are 1.0 in the reference's own arithmetic, and the
demo's argmax then takes the first of them.  The fixture therefore has, in the sentence with four masks, three certain positions
(log-odds 24.6: 1.0 in fp32 on any engine within the tolerance) and one uncertain position (log-odds 8.2: p = 0.9997), which is the
LEFTMOST of the four: the loop must fill the certain ones from left to right (the tie rule) and the leftmost position last (the
probability rule).  The position margin of the fixture is the distance of every candidate's log-odds from SATURATION (its class cannot
change within it), and the gap between two uncertain candidates where they compete.  The solved rows are stored in the fixture (8 x 768 floats per case, row norms about 4); everything else is
seeded.  The VQA head gets its ladder from five raised output biases alone: the pooled features of the three samples of a random two-layer
model are nearly collinear, and rows that told them apart had norms of 50 to 60 - a head whose bf16 error is no longer that of a trained
one.  MARGIN_FACTOR * 0.1 * max(1, |z|max) is the least gap any recorded decision may have."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import rmcl_oracle as O
from tests import mlm_oracle as M
from tests import vqa_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "toy_vocab.txt")
FIXTURE = "predict_L2.npz"
CASES = ("equal", "ragged")
MASK_ID = 103
WORD0, WORD1 = 1000, 1143          # the words of the toy vocabulary (ids [WORD0, WORD1)); the ## pieces behind them are left out
B, N_SPECIAL, TOP_K = 3, 8, 5
N_MASKS = (0, 1, 4)                # masks of the three sentences
BF16_LOGITS_TOL = 0.1              # tests/test_mlm_gpu.py TOL["bf16"]["logits"] (x max(1, |z|max))
MARGIN_FACTOR = 2.0
MLM_TOP, MLM_STEP, MLM_FLOOR = 36.0, 8.2, -33.5
SATURATION = 25 * float(np.log(2.0))   # log-odds beyond which an fp32 probability rounds to exactly 1.0 (1 - p < 2^-25)
CERTAIN, UNCERTAIN = 1, 3              # ladder ranks: the runner-up 3 STEP / 1 STEP below the first place
VQA_TOP, VQA_STEP, VQA_FLOOR = 30.0, 13.5, -36.0
SEEDS = dict(weights=11, mlm_head=75, vqa_head=55, batch=31, design=91)


def config():
    return O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=B)


def make_batch(cfg, case: str):
    """three sentences of toy-vocabulary words with 0, 1 and 4 [MASK] tokens, and per sentence the order in which the loop is to fill
    them: the certain positions from left to right, then - where there are four - the leftmost, uncertain one"""
    ragged = case == "ragged"
    seed = SEEDS["batch"] + CASES.index(case)
    batch = O.synthetic_batch(cfg, B, seed, ragged_text=ragged)
    g = torch.Generator().manual_seed(seed + 1)
    ids, masks = batch["text_ids"], batch["text_masks"]
    words = torch.randint(WORD0, WORD1, ids.shape, generator=g)
    inner = masks.bool() & (ids != 101) & (ids != 102)
    ids[inner] = words[inner]
    order = []
    for b, n in enumerate(N_MASKS):
        pos = torch.nonzero(inner[b]).view(-1)
        pick = sorted(pos[torch.randperm(pos.numel(), generator=g)[:n]].tolist())
        ids[b, pick] = MASK_ID
        order.append(pick[1:] + pick[:1] if n == max(N_MASKS) else pick)
    batch["text_ids"] = ids
    return batch, order


def base_params(cfg):
    return dict(O.init_params(cfg, SEEDS["weights"]), **M.mlm_init_params(cfg, SEEDS["mlm_head"]), **V.vqa_init_params(cfg, SEEDS["vqa_head"]))


def special_ids(case: str):
    """(eight word ids of the toy vocabulary, eight answer ids), seeded per case"""
    g = torch.Generator().manual_seed(SEEDS["design"] + CASES.index(case))
    return (torch.randperm(WORD1 - WORD0, generator=g)[:N_SPECIAL] + WORD0), torch.randperm(V.N_LABELS, generator=g)[:N_SPECIAL]


def floor_heads(p, case: str):
    """the seeded heads with every output bias at FLOOR (+ its seeded N(0, 0.02) value); the special MLM rows' biases at 0; the first five
    special answers' biases on the VQA ladder"""
    p = dict(p)
    tok, ans = special_ids(case)
    b = p["mlm_score.bias"].clone()
    b[b.abs() > 1.0] = 0.0                                                 # (the two raised biases of mlm_oracle.dominant_tokens)
    b = b + MLM_FLOOR
    b[tok] = 0.0
    p["mlm_score.bias"] = b
    b = p["vqa_classifier.3.bias"] + VQA_FLOOR
    b[ans[:TOP_K]] = torch.tensor(ladder(3, VQA_TOP, VQA_STEP))
    p["vqa_classifier.3.bias"] = b
    return p


def with_designed_rows(p, case: str, mlm_rows):
    p = floor_heads(p, case)
    w = p["mlm_score.decoder.weight"].clone()
    w[special_ids(case)[0]] = torch.as_tensor(mlm_rows, dtype=torch.float32)
    p["mlm_score.decoder.weight"] = w
    return p


def ladder(c: int, top: float, step: float):
    """the five prescribed logits of a row of ladder rank c (CERTAIN / UNCERTAIN)"""
    second = top - (4 - c) * step
    return [top] + [second - r * step for r in range(TOP_K - 1)]


def targets(case: str, n_rows: int, ranks):
    """[n_rows, N_SPECIAL] prescribed logits: row j ranks the eight special columns in its own seeded order; places 6 .. 8 sit at the floor"""
    g = torch.Generator().manual_seed(SEEDS["design"] + 17 * CASES.index(case))
    top, step, floor = MLM_TOP, MLM_STEP, MLM_FLOOR
    T = torch.full((n_rows, N_SPECIAL), floor, dtype=torch.float64)
    perms = {}
    for j, (key, c) in enumerate(ranks):
        if key not in perms:
            perms[key] = torch.randperm(N_SPECIAL, generator=g)
        T[j, perms[key][:TOP_K]] = torch.tensor(ladder(c, top, step), dtype=torch.float64)
    return T


def solve_rows(F, T):
    """minimum-norm W [N_SPECIAL, D] with F W^T = T (F [n, D] float64 of full row rank)"""
    return torch.linalg.lstsq(F.double(), T.double()).solution.t().contiguous()


def visited(order):
    """[(round, sentence, position, ladder rank)] of every masked position at every round of the prescribed trajectory"""
    out = []
    for r in range(max(N_MASKS)):
        for b, pick in enumerate(order):
            for i, pos in enumerate(pick):
                if i >= r:
                    out.append((r, b, pos, UNCERTAIN if (len(pick) == max(N_MASKS) and i == len(pick) - 1) else CERTAIN))
    return out


def trajectory_ids(ids, order, tops):
    """ids at the start of every round when the masks go in `order` and position (b, pos) takes the token tops[(b, pos)]"""
    cur, out = ids.clone(), []
    for r in range(max(N_MASKS)):
        out.append(cur.clone())
        for b, pick in enumerate(order):
            if r < len(pick):
                cur[b, pick[r]] = tops[(b, pick[r])]
    return out


def fill_loop(logits_fn, ids, masks, top_k=TOP_K):
    """The demo's loop on ids.  Every round: fp32 softmax over the vocabulary at every position, as the demo takes it; within a sentence,
    among the positions that still hold [MASK], the one whose most likely token has the highest probability (the first on a tie) takes
    that token.  logits_fn(ids) -> [B, L, V] fp32.  Returns (final ids, rounds): per round and sentence with a mask left a dict with the position, the token, its
    probability, the top_k ids / probabilities there, and the logit rows of every masked position (for the margins)."""
    ids = ids.clone()
    rounds = []
    while True:
        live = (ids == MASK_ID) & masks.bool()
        if not bool(live.any()):
            return ids, rounds
        z = logits_fn(ids)
        p = torch.softmax(z.float(), dim=-1)
        best_p, best_tok = p.max(dim=-1)
        this = []
        for b in range(ids.shape[0]):
            if not bool(live[b].any()):
                continue
            cand = torch.where(live[b], best_p[b], torch.full_like(best_p[b], -1.0))
            pos = int(cand.argmax())                                      # (torch's CPU argmax returns the first maximum)
            tp, ti = p[b, pos].topk(top_k)
            this.append(dict(sentence=b, position=pos, token=int(best_tok[b, pos]), prob=float(best_p[b, pos]), top_ids=ti.tolist(),
                             top_probs=tp.tolist(), masked=torch.nonzero(live[b]).view(-1).tolist(), rows=z[b, live[b]].double()))
        for f in this:
            ids[f["sentence"], f["position"]] = f["token"]
        rounds.append(this)


def margins(rounds):
    """(smallest rank gap, smallest position margin, |z|max) over the recorded decisions, in logits.  Rank gap: places j against j + 1,
    j = 1 .. 5, of every masked row.  Position margin, where a sentence has more than one masked position: the distance of every
    candidate's log-odds (log p / (1 - p) of its best token) from SATURATION, and - where no candidate is saturated - the gap between
    the best and the second-best log-odds."""
    rank_gap, pos_gap, zmax = np.inf, np.inf, 0.0
    for this in rounds:
        for f in this:
            z = f["rows"]
            zmax = max(zmax, float(z.abs().max()))
            top = z.topk(TOP_K + 1, dim=1).values
            rank_gap = min(rank_gap, float((top[:, :-1] - top[:, 1:]).min()))
            if z.shape[0] > 1:
                best, arg = z.max(dim=1)
                rest = z.clone()
                rest[torch.arange(z.shape[0]), arg] = -np.inf
                q = (best - torch.logsumexp(rest, dim=1)).sort(descending=True).values
                pos_gap = min(pos_gap, float((q - SATURATION).abs().min()))
                if float(q[0]) < SATURATION:
                    pos_gap = min(pos_gap, float(q[0] - q[1]))
    return rank_gap, pos_gap, zmax


def oracle_logits_fn(p, cfg, batch):
    def fn(ids):
        out = O.infer(p, cfg, ids, batch["text_masks"], batch["image"][0])
        return M.mlm_head(p, out["text_feats"])
    return fn


def load_case(g, case: str):
    """(cfg, params with the designed heads, batch, fill order) of one case of the loaded fixture `g`"""
    cfg = config()
    batch, order = make_batch(cfg, case)
    p = with_designed_rows(base_params(cfg), case, g[f"{case}_mlm_rows"])
    return cfg, p, batch, order
