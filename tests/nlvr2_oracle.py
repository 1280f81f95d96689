"""CPU oracle of the NLVR2 fine-tuning step (test infrastructure): the reference's nlvr2_classifier, 3-row token-type table, hard-label
cross-entropy, compute_nlvr2 / compute_nlvr2_attack and PGDAttack_nlvr2 restated in torch on top of oracle.rmcl_oracle (infer /
layer_norm / gelu_erf).  Also the seeded head weights, the perturbed third token-type row and the synthetic pair batches that
tools/gen_golden_nlvr2.py feeds the reference, so every nlvr2_* fixture is reproducible from (cfg, seeds) without the reference."""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from oracle import rmcl_oracle as O


def nlvr2_param_shapes(cfg: dict) -> List[Tuple[str, Tuple[int, ...]]]:
    """nlvr2_classifier (vilt_module.py:193-200): Linear(2D, 2D), LayerNorm(2D), GELU, Linear(2D, 2)."""
    D2 = 2 * cfg["hidden_size"]
    return [("nlvr2_classifier.0.weight", (D2, D2)), ("nlvr2_classifier.0.bias", (D2,)),
            ("nlvr2_classifier.1.weight", (D2,)), ("nlvr2_classifier.1.bias", (D2,)),
            ("nlvr2_classifier.3.weight", (2, D2)), ("nlvr2_classifier.3.bias", (2,))]


def nlvr2_init_params(cfg: dict, p: Dict[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Seeded head weights (init_weights distribution, objectives.py:1505-1516, with small random biases / LayerNorm terms) and the
    3-row token-type table: rows [0, 1, 1] of the 2-row one (vilt_module.py:201-205), then row 2 moved off row 1 by a seeded offset -
    a pass that wrongly adds row 1 to image_1's tokens then differs measurably."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in nlvr2_param_shapes(cfg):
        if name.endswith("1.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t.float()
    tt = p["token_type_embeddings.weight"]
    row2 = tt[1] + 0.05 * torch.randn(tt.shape[1], generator=g)
    out["token_type_embeddings.weight"] = torch.stack([tt[0], tt[1], row2]).float()
    return out


def synthetic_pairs(cfg: dict, B: int, seed: int, ragged_text: bool = False, sizes0=None, sizes1=None) -> dict:
    """A pair batch in the layout of the NLVR2 collate (image_0 / image_1 views, answers as bools, table_name): text and image_0 from
    O.synthetic_batch(seed), image_1 from O.synthetic_batch(seed + 1000); the first half of the rows is "dev", the rest "test"."""
    b0 = O.synthetic_batch(cfg, B, seed, ragged_text=ragged_text, sizes=sizes0)
    b1 = O.synthetic_batch(cfg, B, seed + 1000, sizes=sizes1)
    g = torch.Generator().manual_seed(seed + 7)
    answers = [bool(x) for x in torch.randint(0, 2, (B,), generator=g).tolist()]
    names = [f"nlvr2_{'dev' if b < (B + 1) // 2 else 'test'}" for b in range(B)]
    return {"image_0": [b0["image"][0]], "image_1": [b1["image"][0]], "text": b0["text"], "text_ids": b0["text_ids"],
            "text_masks": b0["text_masks"], "text_labels": b0["text_labels"], "answers": answers, "table_name": names}


def nlvr2_head(p: Dict[str, torch.Tensor], cls2: torch.Tensor) -> torch.Tensor:
    h = cls2 @ p["nlvr2_classifier.0.weight"].t() + p["nlvr2_classifier.0.bias"]
    h = O.gelu_erf(O.layer_norm(h, p["nlvr2_classifier.1.weight"], p["nlvr2_classifier.1.bias"], 1e-5))
    return h @ p["nlvr2_classifier.3.weight"].t() + p["nlvr2_classifier.3.bias"]


def labels_of(batch) -> torch.Tensor:
    return torch.tensor(batch["answers"]).long()


def forward(p, cfg, batch, img0=None, img1=None):
    """cat([infer(t=1).cls, infer(t=2).cls]) -> nlvr2_classifier (objectives.py:1004-1010)."""
    i0 = batch["image_0"][0] if img0 is None else img0
    i1 = batch["image_1"][0] if img1 is None else img1
    c1 = O.infer(p, cfg, batch["text_ids"], batch["text_masks"], i0, image_token_type_idx=1)["cls_feats"]
    c2 = O.infer(p, cfg, batch["text_ids"], batch["text_masks"], i1, image_token_type_idx=2)["cls_feats"]
    return nlvr2_head(p, torch.cat([c1, c2], dim=-1))


def compute_nlvr2(p, cfg, batch, img0=None, img1=None) -> dict:
    logits = forward(p, cfg, batch, img0, img1)
    labels = labels_of(batch)
    return {"nlvr2_loss": F.cross_entropy(logits, labels), "nlvr2_logits": logits, "nlvr2_labels": labels}


def pgd_attack(p, cfg, batch, attack_idx, return_prev: bool = False):
    """PGDAttack_nlvr2.pgd_attack (pgd_attack_vilt.py:259-342): K steps, loss CE / K, per attacked image
    delta <- clamp(delta + lr g / max(|g|_inf, 1e-8), +-eps); a non-attacked image keeps delta 0."""
    K, lr, eps = cfg["adv_steps_img"], cfg["adv_lr_img"], cfg["adv_max_norm_img"]
    i0, i1 = batch["image_0"][0], batch["image_1"][0]
    d = [torch.zeros_like(i0), torch.zeros_like(i1)]
    prev = [x.clone() for x in d]
    labels = labels_of(batch)
    for _ in range(K):
        prev = [x.clone() for x in d]
        x = [d[k].detach().clone().requires_grad_(bool(attack_idx[k])) for k in range(2)]
        with torch.enable_grad():
            loss = F.cross_entropy(forward(p, cfg, batch, i0 + x[0], i1 + x[1]), labels) / K
            wrt = [x[k] for k in range(2) if attack_idx[k]]
            grads = torch.autograd.grad(loss, wrt)
        gi = iter(grads)
        for k in range(2):
            if not attack_idx[k]:
                continue
            g = next(gi)
            den = g.abs().flatten(1).max(dim=1).values.clamp_min(1e-8).view(-1, 1, 1, 1)
            nd = d[k] + lr * g / den
            d[k] = (nd.clamp(-eps, eps) if eps > 0 else nd).detach()
    return (d, prev) if return_prev else d


def compute_nlvr2_attack(p, cfg, batch, attack_idx) -> dict:
    """compute_nlvr2_attack (objectives.py:898-1000), image view: clean pair, then the attacked pair on img + delta_{K-1} + delta_K."""
    clean = compute_nlvr2(p, cfg, batch)
    d, prev = pgd_attack(p, cfg, batch, attack_idx, return_prev=True)
    att = compute_nlvr2(p, cfg, batch, batch["image_0"][0] + prev[0] + d[0], batch["image_1"][0] + prev[1] + d[1])
    log = (torch.linalg.norm(d[0], dim=1).mean() + torch.linalg.norm(d[1], dim=1).mean()) / sum(bool(a) for a in attack_idx)
    return {"nlvr2_original_logits": clean["nlvr2_logits"], "nlvr2_original_loss": clean["nlvr2_loss"],
            "nlvr2_attacked_logits": att["nlvr2_logits"], "nlvr2_attacked_loss": att["nlvr2_loss"], "nlvr2_labels": clean["nlvr2_labels"],
            "delta0": d[0], "delta1": d[1], "delta_log": log}


# (name, B, seed_w, seed_h, seed_b, layers, K, attack_idx or None, ragged sizes of image_0 / image_1 or None)
CASES = {
    "nlvr2_L2_B4_ragged": (4, 11, 71, 31, 2, 1, None, [(384, 320), (256, 384), (320, 320), (384, 384)],
                           [(320, 384), (384, 256), (288, 352), (352, 224)]),
    "nlvr2_L12_B2": (2, 12, 72, 32, 12, 1, None, None, None),
    "nlvr2_att_K2_L2_B4": (4, 13, 73, 33, 2, 2, (True, True), None, None),
    "nlvr2_att_K2_L2_B4_idx10": (4, 13, 74, 34, 2, 2, (True, False), None, None),
}
FIXTURES = tuple(CASES)


def case_inputs(name: str):
    """(cfg, params incl. head and 3-row token types, batch, attack_idx) of a fixture, from its seeds alone."""
    B, sw, sh, sb, L, K, idx, s0, s1 = CASES[name]
    cfg = O.default_config(num_layers=L, num_negative=1024, adv_steps_img=K, per_gpu_batchsize=B)
    p = O.init_params(cfg, sw)
    p.update(nlvr2_init_params(cfg, p, sh))
    batch = synthetic_pairs(cfg, B, sb, ragged_text=True, sizes0=s0, sizes1=s1)
    return cfg, p, batch, idx


def load_case(name: str):
    from tests.golden_util import load
    g = load(name + ".npz")
    cfg, p, batch, idx = case_inputs(name)
    return g, cfg, p, batch, idx
