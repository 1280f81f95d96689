"""Generate the masked-language-modelling golden fixtures tests/golden/mlm_*.npz by running the REFERENCE's own compute_mlm
(vilt/modules/objectives.py:604-630) - and compute_itm_wpa for the combined case - on the reference's own heads.MLMHead(bert_config)
(vilt_module.py:56: no tied weight).

TEST INFRASTRUCTURE ONLY: runs on the build machine only (needs the reference checkout that oracle/gen_golden.py imports).  It imports
oracle.gen_golden (its stand-ins, Holder - whose infer(**kw) forwards mask_text -, tensor_digest) and oracle.rmcl_oracle unchanged; the
head weights and the masking come from tests/mlm_oracle.py (seeded), so every fixture is reproducible without the reference and the
94 MB decoder.weight is never stored.

Every fixture is checked here, on the CPU, for near ties: no masked row of the reference may have a top-two logit gap below the bf16
logits tolerance (0.1 x max(1, |z|max)) - the GPU test's exemption for such rows then cannot hide a wrong argmax.

Usage:  python tools/gen_golden_mlm.py      (writes tests/golden/mlm_*.npz and mlm_head_shapes.json, a few minutes)
"""
from __future__ import annotations

import json
import os
import sys
from copy import deepcopy

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins, imports the reference)
from oracle import rmcl_oracle as O  # noqa: E402
from tests import golden_util  # noqa: E402
from tests import mlm_oracle as M  # noqa: E402

NEAR_TIE = 0.1          # the bf16 logits tolerance of tests/test_mlm_gpu.py


def _accuracy(logits, target):
    """Accuracy.update + compute for one batch (gadgets/my_metrics.py:5-28; its Metric base class is a stand-in here)."""
    logits, target = logits.detach(), target.detach()
    preds = logits.argmax(dim=-1)
    preds = preds[target != -100]
    target = target[target != -100]
    if target.numel() == 0:
        return torch.tensor(float("nan"))
    return (preds == target).sum().float() / target.numel()


def make_holder(cfg):
    h = G.Holder(cfg)
    bc = G.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_layers"],
                      num_attention_heads=cfg["num_heads"], intermediate_size=cfg["hidden_size"] * cfg["mlp_ratio"],
                      max_position_embeddings=cfg["max_text_len"], hidden_dropout_prob=cfg["drop_rate"],
                      attention_probs_dropout_prob=cfg["drop_rate"])
    h.mlm_score = G.heads.MLMHead(bc)
    for phase in ("train", "val"):
        setattr(h, f"{phase}_mlm_loss", lambda x: x)
        setattr(h, f"{phase}_mlm_accuracy", _accuracy)
    return h


def run_mlm(tag, cfg, B, seed_w, seed_h, seed_b, seed_m, ragged, mode, with_itm):
    torch.manual_seed(999)
    cfg = dict(cfg, per_gpu_batchsize=B)
    p = dict(O.init_params(cfg, seed_w), **M.mlm_init_params(cfg, seed_h))
    h = make_holder(cfg)
    h.load_oracle_params(p)
    h.train()
    batch = O.synthetic_batch(cfg, B, seed_b, ragged_text=ragged)
    batch = M.synthetic_mlm(batch, seed_m, cfg["vocab_size"], mode, dup_label=M.dominant_tokens(cfg, seed_h)[0])
    h.zero_grad()
    ret = G.objectives.compute_mlm(h, deepcopy(batch))
    loss = ret["mlm_loss"]
    out = {}
    if with_itm:
        r2 = G.objectives.compute_itm_wpa(h, deepcopy(batch))
        loss = loss + r2["itm_loss"] + r2["itm_wpa_loss"]
        out.update(itm_loss=np.float64(r2["itm_loss"].item()), itm_wpa_loss=np.float64(r2["itm_wpa_loss"].item()),
                   itm_labels=r2["itm_labels"].numpy(), total_loss=np.float64(loss.item()))
    loss.backward()
    labels = batch["text_labels_mlm"]
    on = labels != -100
    n = int(on.sum())
    logits = ret["mlm_logits"].detach()
    assert logits.shape == (B, cfg["max_text_len"], cfg["vocab_size"])
    rows = logits[on]                                                   # [n, V], ascending (b, l)
    lab = labels[on]
    top2 = rows.topk(2, dim=1).values if n else torch.zeros(0, 2)
    gap = top2[:, 0] - top2[:, 1]
    zmax = float(rows.abs().max()) if n else 0.0
    assert n == 0 or float(gap.min()) >= NEAR_TIE * max(1.0, zmax), (tag, float(gap.min()), zmax)      # no near-tie row: re-seed if this fires
    cols = M.sample_columns(cfg, seed_h, labels)
    argmax = rows.argmax(dim=1) if n else torch.zeros(0, dtype=torch.int64)
    out.update(mlm_loss=np.float64(ret["mlm_loss"].item()), n=np.int64(n), correct=np.int64(int((argmax == lab).sum())),
               log_accuracy=np.float64(h.logged["mlm/train/accuracy"]), log_loss=np.float64(h.logged["mlm/train/loss"]),
               row_loss=torch.nn.functional.cross_entropy(rows, lab, reduction="none").numpy() if n else np.zeros(0, np.float32),
               argmax=argmax.numpy(), gap=gap.numpy(), zmax=np.float64(zmax), sample_cols=cols.numpy(),
               sample_logits=rows[:, cols].numpy(), labels=lab.numpy(),
               ids_mlm_digest=G.tensor_digest(ret["mlm_ids"].float()), text_feats_digest=np.zeros(0))
    gnames, gd = [], []
    for name, prm in h.named_parameters():
        if not name.startswith("k_") and prm.grad is not None:
            gnames.append(name)
            gd.append(G.tensor_digest(prm.grad))
    out["grad_names"] = np.array(gnames)
    out["grad_digest"] = np.stack(gd)
    ms = h.mlm_score
    out["grad_decoder_w"] = ms.decoder.weight.grad[cols[:16], :64].numpy().copy()
    out["grad_mlm_bias"] = ms.bias.grad[cols].numpy().copy()
    out["grad_dense_w"] = ms.transform.dense.weight.grad[:8, :64].numpy().copy()
    out["grad_ln_w"] = ms.transform.LayerNorm.weight.grad[:64].numpy().copy()
    out["grad_ln_b"] = ms.transform.LayerNorm.bias.grad[:64].numpy().copy()
    out["grad_dense_b"] = ms.transform.dense.bias.grad[:64].numpy().copy()
    wrows = torch.tensor([M.MASK_ID, 101, 102] + batch["text_ids_mlm"][:, 1].tolist(), dtype=torch.int64)
    out["word_rows"] = wrows.numpy()
    out["grad_word"] = h.text_embeddings.word_embeddings.weight.grad[wrows, :64].numpy().copy()
    out["grad_qkv0_w"] = h.transformer.blocks[0].attn.qkv.weight.grad[:8, :64].numpy().copy()
    out["meta"] = np.array([B, seed_w, seed_h, seed_b, seed_m, int(ragged), cfg["num_layers"], M.MODES.index(mode), int(with_itm)], dtype=np.int64)
    del out["text_feats_digest"]
    path = os.path.join(ROOT, "tests", "golden", f"{tag}.npz")
    golden_util.save(path, out)
    print(os.path.basename(path), "loss", out["mlm_loss"], "n", n, "correct", int(out["correct"]), "min gap", float(gap.min()) if n else None,
          "zmax", zmax, "bytes", os.path.getsize(path))
    return h


if __name__ == "__main__":
    torch.set_num_threads(16)
    small = O.default_config(num_layers=2, num_negative=1024)
    full = O.default_config()
    h = run_mlm("mlm_L2_B4_ragged", small, 4, 11, 71, 21, 81, True, "ragged", False)
    shapes = {k: list(v.shape) for k, v in h.state_dict().items() if k.startswith("mlm_score.")}
    with open(os.path.join(ROOT, "tests", "golden", "mlm_head_shapes.json"), "w") as f:
        json.dump(shapes, f, indent=1)
    run_mlm("mlm_itm_L2_B4", small, 4, 11, 72, 23, 82, True, "random", True)
    run_mlm("mlm_L2_B2_empty", small, 2, 11, 73, 24, 83, False, "empty", False)
    run_mlm("mlm_L12_B2", full, 2, 12, 74, 22, 84, False, "random", False)
