"""CPU oracle of the VQAv2 fine-tuning step (test infrastructure): the reference's vqa_classifier, soft-target BCE, VQAScore and
PGDAttack_vqa restated in torch on top of oracle.rmcl_oracle (infer / layer_norm / gelu_erf).  Also the seeded head weights and
synthetic label / score lists that tools/gen_golden_vqa.py feeds the reference, so every vqa_* fixture is reproducible from
(cfg, seeds) without the reference."""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from oracle import rmcl_oracle as O

N_LABELS = 3129          # vqav2_label_size (reference config.py:53)


def vqa_param_shapes(cfg: dict) -> List[Tuple[str, Tuple[int, ...]]]:
    """vqa_classifier (vilt_module.py:166-171): Linear(D, 2D), LayerNorm(2D), GELU, Linear(2D, vqav2_label_size)."""
    D, N = cfg["hidden_size"], cfg.get("vqav2_label_size", N_LABELS)
    return [("vqa_classifier.0.weight", (2 * D, D)), ("vqa_classifier.0.bias", (2 * D,)),
            ("vqa_classifier.1.weight", (2 * D,)), ("vqa_classifier.1.bias", (2 * D,)),
            ("vqa_classifier.3.weight", (N, 2 * D)), ("vqa_classifier.3.bias", (N,))]


def vqa_init_params(cfg: dict, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded head weights for the fixtures: the reference's init_weights distribution (objectives.py:1505-1516: Linear N(0, 0.02),
    LayerNorm 1 / 0), with small random biases and LayerNorm affine terms so that their gradients are exercised off the init point."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in vqa_param_shapes(cfg):
        if name.endswith("1.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 2:
            t = 0.02 * torch.randn(shape, generator=g)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t.float()
    return out


def synthetic_labels(B: int, seed: int, N: int = N_LABELS) -> Tuple[list, list]:
    """Per-sample answer lists like the VQAv2 collate (lists of label ids / soft scores): row 0 is empty, row 1 repeats a label
    (the later score wins), row 2 has 10 answers (row 1 when B == 2); further rows 1-5 answers."""
    g = torch.Generator().manual_seed(seed)
    labels, scores = [], []
    first = [0, 10] if B == 2 else [0, 4, 10]
    for b in range(B):
        n = first[b] if b < len(first) else int(torch.randint(1, 6, (1,), generator=g))
        ls = torch.randint(0, N, (n,), generator=g).tolist()
        ss = [round(float(x), 4) for x in torch.rand(n, generator=g)]
        if b == 1 and n >= 3:
            ls[2] = ls[0]                               # duplicate: target[l] = the score of the LAST occurrence
        labels.append(ls)
        scores.append(ss)
    return labels, scores


def dense_targets(labels, scores, B: int, N: int = N_LABELS, dtype=torch.float32) -> torch.Tensor:
    """objectives.py:871-877: the list-order fill (a repeated label keeps its last score)."""
    t = torch.zeros(B, N, dtype=dtype)
    for i, (ls, ss) in enumerate(zip(labels, scores)):
        for l, s in zip(ls, ss):
            t[i, l] = s
    return t


def vqa_head(p: Dict[str, torch.Tensor], cls: torch.Tensor) -> torch.Tensor:
    """vqa_classifier forward (vilt_module.py:166-171): LayerNorm eps 1e-5, exact-erf GELU."""
    h = cls @ p["vqa_classifier.0.weight"].t() + p["vqa_classifier.0.bias"]
    h = O.gelu_erf(O.layer_norm(h, p["vqa_classifier.1.weight"], p["vqa_classifier.1.bias"], 1e-5))
    return h @ p["vqa_classifier.3.weight"].t() + p["vqa_classifier.3.bias"]


def vqa_loss(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """objectives.py:879-882: BCE-with-logits (mean) x vqav2_label_size."""
    return F.binary_cross_entropy_with_logits(logits, targets) * targets.shape[1]


def vqa_score(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """VQAScore.update + compute for one batch (gadgets/my_metrics.py:65-85): targets[b, argmax_b] summed / B."""
    idx = logits.argmax(dim=1)
    return targets.gather(1, idx.view(-1, 1)).sum() / logits.shape[0]


def forward(p, cfg, batch, img=None):
    out = O.infer(p, cfg, batch["text_ids"], batch["text_masks"], batch["image"][0] if img is None else img)
    return vqa_head(p, out["cls_feats"])


def compute_vqa(p, cfg, batch, targets, img=None) -> dict:
    """compute_vqa (objectives.py:861-896) on `img` (default: the batch image)."""
    logits = forward(p, cfg, batch, img)
    loss = vqa_loss(logits, targets)
    return {"vqa_loss": loss, "vqa_logits": logits, "vqa_score": vqa_score(logits.detach(), targets)}


def pgd_attack(p, cfg, batch, targets, return_steps: bool = False):
    """PGDAttack_vqa.pgd_attack (attack/pgd_attack_vilt.py:433-483): K steps of delta <- clamp(delta + lr g / max(|g|_inf, 1e-8), +-eps),
    g = d(BCE x N)/d delta (NOT divided by K).  Only the data gradient is formed (the leaked weight gradients: INTEGRATION.md)."""
    K, lr, eps = cfg["adv_steps_img"], cfg["adv_lr_img"], cfg["adv_max_norm_img"]
    img0 = batch["image"][0]
    delta = torch.zeros_like(img0)
    steps = []
    for _ in range(K):
        d = delta.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            loss = vqa_loss(forward(p, cfg, batch, img0 + d), targets)
            (g,) = torch.autograd.grad(loss, d)
        den = g.abs().flatten(1).max(dim=1).values.clamp_min(1e-8).view(-1, 1, 1, 1)
        delta = delta + lr * g / den
        if eps > 0:
            delta = delta.clamp(-eps, eps)
        delta = delta.detach()
        steps.append(delta.clone())
    return (delta, steps) if return_steps else delta


def compute_vqa_attack(p, cfg, batch, targets) -> dict:
    """compute_vqa_attack (objectives.py:813-859), image view: the attacked view is img + delta_{K-1} + delta_K (compute_pgd :176 on
    top of the batch image pgd_attack leaves behind, :444)."""
    delta, steps = pgd_attack(p, cfg, batch, targets, return_steps=True)
    prev = steps[-2] if len(steps) > 1 else torch.zeros_like(delta)
    img = batch["image"][0] + prev + delta
    out = compute_vqa(p, cfg, batch, targets, img=img)
    out["delta"] = delta
    out["delta_log"] = torch.linalg.norm(delta, dim=1).mean()
    return out


FIXTURES = ("vqa_L2_B4_ragged", "vqa_att_K2_L2_B4_ragged", "vqa_L12_B2")


def load_case(name: str):
    """A vqa_* fixture with everything needed to recompute it: (fixture, cfg, params incl. the head, batch with vqa_labels /
    vqa_scores, dense targets, attacked?)."""
    from tests.golden_util import load
    g = load(name + ".npz")
    B, sw, sh, sb, sl, ragged, L, K = [int(x) for x in g["meta"]]
    cfg = O.default_config(num_layers=L, num_negative=1024 if L == 2 else 65536, adv_steps_img=K, per_gpu_batchsize=B,
                           vqav2_label_size=N_LABELS)
    p = dict(O.init_params(cfg, sw), **vqa_init_params(cfg, sh))
    batch = O.synthetic_batch(cfg, B, sb, ragged_text=bool(ragged))
    labels, scores = synthetic_labels(B, sl)
    assert [len(r) for r in labels] == g["labels_len"].tolist()
    batch["vqa_labels"], batch["vqa_scores"] = labels, scores
    batch["qid"] = list(range(B))
    return g, cfg, p, batch, dense_targets(labels, scores, B), "_att_" in name
