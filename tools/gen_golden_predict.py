"""Generate the prediction fixture tests/golden/predict_L2.npz by running the REFERENCE's own model (its BertEmbeddings, VisionTransformer,
Pooler through oracle.gen_golden.Holder), its heads.MLMHead and its nn.Sequential VQA head on the toy vocabulary, L = 2 layers, B = 3
sentences with 0, 1 and 4 [MASK] tokens - once with equal text lengths and once ragged.

TEST INFRASTRUCTURE ONLY: runs on the build machine only, on the CPU (needs the reference checkout that oracle/gen_golden.py imports).  It
imports oracle.gen_golden and oracle.rmcl_oracle unchanged.  The mask-filling loop of the reference's demo is nested inside its main() and
cannot be imported; tests/predict_oracle.py restates it on ids (fill_loop), and this tool runs that loop with the reference's modules
producing the logits.  Batch, encoder weights and the heads' seeded parts come from tests/predict_oracle.py / mlm_oracle.py /
vqa_oracle.py; the eight designed rows of mlm_score.decoder (predict_oracle's docstring) are solved HERE on the reference's own features
and stored.

Margin condition: no test may skip a decision, so the generator refuses a seed in which a recorded decision has a margin below twice the
bf16 logits tolerance of tests/test_mlm_gpu.py (0.1 * max(1, |z|max)): places j against j + 1 of a masked row for j = 1 .. 5, the VQA
places likewise, and for the chosen position the margin of tests/predict_oracle.py (the demo compares fp32 probabilities, which are
exactly 1.0 beyond 17.33 logits of log-odds: every candidate's distance from that threshold, and the gap between unsaturated rivals).
The smallest margins found are stored.

Usage:  python tools/gen_golden_predict.py      (writes tests/golden/predict_L2.npz, under a minute)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins, imports the reference)
from tests import golden_util  # noqa: E402
from tests import predict_oracle as PO  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402


def make_holder(cfg, p):
    h = G.Holder(cfg)
    bc = G.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_layers"],
                      num_attention_heads=cfg["num_heads"], intermediate_size=cfg["hidden_size"] * cfg["mlp_ratio"],
                      max_position_embeddings=cfg["max_text_len"], hidden_dropout_prob=cfg["drop_rate"],
                      attention_probs_dropout_prob=cfg["drop_rate"])
    D = cfg["hidden_size"]
    h.mlm_score = G.heads.MLMHead(bc)
    h.vqa_classifier = nn.Sequential(nn.Linear(D, 2 * D), nn.LayerNorm(2 * D), nn.GELU(), nn.Linear(2 * D, V.N_LABELS))
    h.load_oracle_params(p)
    h.eval()
    return h


def infer(h, batch, ids):
    with torch.no_grad():
        return h.infer(dict(batch, text_ids=ids))


def run_case(case, out):
    cfg = PO.config()
    batch, order = PO.make_batch(cfg, case)
    ids0, masks = batch["text_ids"].clone(), batch["text_masks"]
    tok, ans = PO.special_ids(case)
    p0 = PO.floor_heads(PO.base_params(cfg), case)
    h = make_holder(cfg, p0)

    # the rows the loop will visit under the prescribed order, and the token each position is to take
    vis = PO.visited(order)
    T = PO.targets(case, len(vis), [((b, pos), c) for _, b, pos, c in vis])
    tops = {(b, pos): int(tok[int(T[j].argmax())]) for j, (_, b, pos, _) in enumerate(vis)}
    feats = []
    for r, ids in enumerate(PO.trajectory_ids(ids0, order, tops)):
        tf = infer(h, batch, ids)["text_feats"]
        with torch.no_grad():
            feats += [h.mlm_score.transform(tf[b, pos]) for rr, b, pos, _ in vis if rr == r]
    mlm_rows = PO.solve_rows(torch.stack(feats), T).float()

    h = make_holder(cfg, PO.with_designed_rows(PO.base_params(cfg), case, mlm_rows))

    def logits_fn(ids):
        with torch.no_grad():
            return h.mlm_score(infer(h, batch, ids)["text_feats"])

    final, rounds = PO.fill_loop(logits_fn, ids0, masks)
    rank_gap, pos_gap, zmax = PO.margins(rounds)
    need = PO.MARGIN_FACTOR * PO.BF16_LOGITS_TOL * max(1.0, zmax)
    assert rank_gap >= need and pos_gap >= need, (case, rank_gap, pos_gap, need)         # re-seed (predict_oracle.SEEDS) if this fires
    fills = [(r, f["sentence"], f["position"], f["token"]) for r, this in enumerate(rounds) for f in this]
    got_order = [[f[2] for f in fills if f[1] == b] for b in range(PO.B)]
    assert got_order == order and all(tops[(f[1], f[2])] == f[3] for f in fills), (got_order, order)    # the loop took the prescribed path
    assert len(rounds) == max(PO.N_MASKS) and not bool((final == PO.MASK_ID).any())

    with torch.no_grad():
        z = h.vqa_classifier(infer(h, batch, ids0)["cls_feats"]).double()
    vt = z.topk(PO.TOP_K + 1, dim=1)
    vgap, vzmax = float((vt.values[:, :-1] - vt.values[:, 1:]).min()), float(z.abs().max())
    assert vgap >= PO.MARGIN_FACTOR * PO.BF16_LOGITS_TOL * max(1.0, vzmax), (case, vgap, vzmax)

    flat = [f for this in rounds for f in this]
    out.update({
        f"{case}_mlm_rows": mlm_rows.numpy(),
        f"{case}_ids0": ids0.numpy(), f"{case}_masks": masks.numpy(), f"{case}_final_ids": final.numpy(),
        f"{case}_fills": np.array(fills, dtype=np.int64), f"{case}_fill_prob": np.array([f["prob"] for f in flat]),
        f"{case}_top_ids": np.array([f["top_ids"] for f in flat], dtype=np.int64), f"{case}_top_probs": np.array([f["top_probs"] for f in flat]),
        f"{case}_margins": np.array([rank_gap, pos_gap, zmax]),
        f"{case}_vqa_top_ids": vt.indices[:, : PO.TOP_K].numpy(), f"{case}_vqa_top_logits": vt.values[:, : PO.TOP_K].numpy(),
        f"{case}_vqa_margins": np.array([vgap, vzmax]),
    })
    print(case, "fills", fills, "rank gap %.3f position gap %.3f |z|max %.3f (need %.3f)" % (rank_gap, pos_gap, zmax, need),
          "vqa gap %.3f |z|max %.3f" % (vgap, vzmax), "largest row norm %.2f" % float(mlm_rows.norm(dim=1).max()))


if __name__ == "__main__":
    torch.set_num_threads(16)
    out = {"meta": np.array([PO.SEEDS[k] for k in ("weights", "mlm_head", "vqa_head", "batch", "design")], dtype=np.int64)}
    for case in PO.CASES:
        run_case(case, out)
    path = os.path.join(ROOT, "tests", "golden", PO.FIXTURE)
    golden_util.save(path, out)
    print(os.path.basename(path), "bytes", os.path.getsize(path))
