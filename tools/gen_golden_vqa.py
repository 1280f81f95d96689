"""Generate the VQAv2 golden fixtures tests/golden/vqa_*.npz by running the REFERENCE's own compute_vqa / compute_vqa_attack /
PGDAttack_vqa (vilt/modules/objectives.py:813-896, attack/pgd_attack_vilt.py:418-483) and its nn.Sequential head (vilt_module.py:166-172).

TEST INFRASTRUCTURE ONLY: runs on the build machine only (needs the reference checkout that oracle/gen_golden.py imports).  It imports
oracle.gen_golden (its stand-ins, Holder, tensor_digest) and oracle.rmcl_oracle (init_params, synthetic_batch) unchanged; the head
weights and the label / score lists come from tests/vqa_oracle.py (seeded), so every fixture is reproducible without the reference.

PGD weight gradients: PGDAttack_vqa back-propagates through the LIVE module, so every PGD step leaves weight gradients in .grad.  Under the
reference's recipe (precision=16, native AMP) they are unscaled and vanish behind the loss scale; the engine forms none.
The generator therefore zeroes the live gradients right after pgd_attack returns and records the leaked part separately
(grad_digest_with_pgd_leak: the digests of the gradients the fp32 reference would have stepped with).

Usage:  python tools/gen_golden_vqa.py      (writes tests/golden/vqa_*.npz, ~1 min)
"""
from __future__ import annotations

import os
import sys
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins, imports the reference)
from oracle import rmcl_oracle as O  # noqa: E402
from attack.pgd_attack_vilt import PGDAttack_vqa  # noqa: E402  (reference, unmodified)
from tests import golden_util  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402

def _score(logits, targets):
    """VQAScore.update + compute for one batch (gadgets/my_metrics.py:65-85; its Metric base class is a stand-in here)."""
    idx = torch.max(logits.detach().float(), 1)[1]
    one_hots = torch.zeros(*targets.size()).to(targets)
    one_hots.scatter_(1, idx.view(-1, 1), 1)
    return (one_hots * targets).sum() / len(idx)


def run_vqa(tag, cfg, B, seed_w, seed_h, seed_b, seed_l, ragged, attacked):
    torch.manual_seed(888)
    cfg = dict(cfg, per_gpu_batchsize=B, vqav2_label_size=V.N_LABELS, image_view=True, text_view=False)
    p = O.init_params(cfg, seed_w)
    hp = V.vqa_init_params(cfg, seed_h)
    h = G.Holder(cfg)
    D = cfg["hidden_size"]
    h.vqa_classifier = nn.Sequential(nn.Linear(D, 2 * D), nn.LayerNorm(2 * D), nn.GELU(), nn.Linear(2 * D, V.N_LABELS))
    h.image_view, h.text_view = True, False
    h.pgd_attacker = PGDAttack_vqa(cfg)
    for phase in ("train", "val"):
        for task in ("vqa", "vqa_attacked"):
            setattr(h, f"{phase}_{task}_loss", lambda x: x)
            setattr(h, f"{phase}_{task}_score", _score)
    h.load_oracle_params(dict(p, **hp))
    h.train()
    batch = O.synthetic_batch(cfg, B, seed_b, ragged_text=ragged)
    labels, scores = V.synthetic_labels(B, seed_l)
    batch["vqa_labels"], batch["vqa_scores"] = labels, scores
    params = [(n, prm) for n, prm in h.named_parameters() if not n.startswith("k_")]
    leak, deltas, prevs = {}, [], []
    attack = h.pgd_attacker.pgd_attack

    def recording_attack(pl_module, b_, **kw):
        d = attack(pl_module, b_, **kw)
        deltas.append(d.detach().clone())
        prevs.append(b_["image"][0].detach().clone() - batch["image"][0])      # img + delta_{K-1} left behind (:444)
        for n, prm in params:                                                    # decision 1: the leaked weight gradients are not stepped
            if prm.grad is not None:
                leak[n] = prm.grad.detach().clone()
                prm.grad = None
        return d

    h.pgd_attacker.pgd_attack = recording_attack
    h.zero_grad()
    fn = G.objectives.compute_vqa_attack if attacked else G.objectives.compute_vqa
    ret = fn(h, deepcopy(batch))
    ret["vqa_loss"].backward()
    out = {"vqa_loss": np.float64(ret["vqa_loss"].item()), "vqa_logits": ret["vqa_logits"].detach().numpy(),
           "vqa_targets_digest": G.tensor_digest(ret["vqa_targets"]),
           "labels_flat": np.array([l for r in labels for l in r], dtype=np.int64),
           "labels_len": np.array([len(r) for r in labels], dtype=np.int64),
           "scores_flat": np.array([s for r in scores for s in r], dtype=np.float32)}
    for kk, v in h.logged.items():
        out["log_" + kk.replace("/", "__")] = np.float64(v)
    gnames, gd, gl = [], [], []
    for n, prm in params:
        if prm.grad is not None:
            gnames.append(n)
            gd.append(G.tensor_digest(prm.grad))
            gl.append(G.tensor_digest(prm.grad + leak[n]) if n in leak else G.tensor_digest(prm.grad))
    out["grad_names"] = np.array(gnames)
    out["grad_digest"] = np.stack(gd)
    if attacked:
        assert len(deltas) == 1 and leak
        out["grad_digest_with_pgd_leak"] = np.stack(gl)
        d = deltas[0]
        out["delta_sub"] = d[:, :, ::8, ::8].contiguous().numpy()
        out["delta_digest"] = G.tensor_digest(d)
        out["delta_patch00"] = d[:, :, :32, :32].contiguous().numpy()
        out["prev_digest"] = G.tensor_digest(prevs[0])
    hc = h.vqa_classifier
    out["grad_vqa_w0"] = hc[0].weight.grad[:8, :64].numpy().copy()
    out["grad_vqa_b0"] = hc[0].bias.grad[:64].numpy().copy()
    out["grad_vqa_g1"] = hc[1].weight.grad[:64].numpy().copy()
    out["grad_vqa_b1"] = hc[1].bias.grad[:64].numpy().copy()
    out["grad_vqa_w3"] = hc[3].weight.grad[:8, :64].numpy().copy()
    out["grad_vqa_b3"] = hc[3].bias.grad[:64].numpy().copy()
    out["grad_pooler_w"] = h.pooler.dense.weight.grad[:8, :64].numpy().copy()
    out["grad_qkv0_w"] = h.transformer.blocks[0].attn.qkv.weight.grad[:8, :64].numpy().copy()
    out["meta"] = np.array([B, seed_w, seed_h, seed_b, seed_l, int(ragged), cfg["num_layers"], cfg["adv_steps_img"]], dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", f"vqa_{'att_' if attacked else ''}{tag}.npz")
    golden_util.save(path, out)
    print(os.path.basename(path), "loss", out["vqa_loss"], {k: v for k, v in out.items() if k.startswith("log_")})


if __name__ == "__main__":
    torch.set_num_threads(8)
    small = O.default_config(num_layers=2, num_negative=1024)
    full = O.default_config()
    run_vqa("L2_B4_ragged", small, 4, 11, 51, 21, 61, True, False)
    run_vqa("K2_L2_B4_ragged", dict(small, adv_steps_img=2), 4, 11, 52, 21, 62, True, True)
    run_vqa("L12_B2", full, 2, 12, 53, 22, 63, False, False)
