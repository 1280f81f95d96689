"""CPU oracle of image-text retrieval (test infrastructure): the reference's rank_output alias (vilt_module.py:233-239), compute_irtr and
compute_irtr_recall (objectives.py:1180-1346) restated in torch on top of oracle.rmcl_oracle, and the seeded inputs that
tools/gen_golden_irtr.py feeds the reference, so every irtr* fixture is reproducible from (cfg, seeds) without the reference."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import rmcl_oracle as O

LR, WD = 1e-4, 0.01                       # the optimizer of the two-step fixture (base learning rate / weight decay of the IRTR configs)


def synthetic_text(cfg: dict, n: int, seed: int):
    """n ragged captions in the layout of O.synthetic_batch(ragged_text=True): ([n, L] ids, masks, labels)."""
    g = torch.Generator().manual_seed(seed)
    Lt = cfg["max_text_len"]
    ids = torch.randint(1000, cfg["vocab_size"], (n, Lt), generator=g, dtype=torch.int64)
    masks = torch.ones(n, Lt, dtype=torch.int64)
    lens = torch.randint(8, Lt + 1, (n,), generator=g)
    for b in range(n):
        k = int(lens[b])
        masks[b, k:] = 0
        ids[b, k:] = 0
        ids[b, k - 1] = 102
    ids[:, 0] = 101
    return ids, masks, torch.full((n, Lt), -100, dtype=torch.int64)


def irtr_batch(cfg: dict, B: int, Fn: int, seed: int, sizes=None) -> dict:
    """A batch in the layout of BaseDataset.collate with draw_false_text = Fn: O.synthetic_batch + false_text_{i}_{ids,masks,labels}."""
    b = O.synthetic_batch(cfg, B, seed, ragged_text=True, sizes=sizes)
    for i in range(Fn):
        ids, masks, labels = synthetic_text(cfg, B, seed + 100 + i)
        b[f"false_text_{i}_ids"], b[f"false_text_{i}_masks"], b[f"false_text_{i}_labels"] = ids, masks, labels
        b[f"false_text_{i}"] = ["synthetic"] * B
    return b


def rank_output(p: Dict[str, torch.Tensor], cls: torch.Tensor, w=None, b=None) -> torch.Tensor:
    """rank_output(cls)[:, 0]: Linear(D, 1) whose weight / bias are row 1 of itm_score.fc (vilt_module.py:233-236)."""
    w = p["itm_score.fc.weight"][1:] if w is None else w
    b = p["itm_score.fc.bias"][1:] if b is None else b
    return (cls @ w.t() + b)[:, 0]


def compute_irtr(p, cfg, batch, w=None, b=None) -> dict:
    """objectives.py:1180-1223: B * (F + 1) sequences (true caption first), scores [B, F + 1], cross-entropy against answer 0."""
    Fn = cfg["draw_false_text"]
    img = batch["image"][0]
    B = img.shape[0]
    ids = torch.stack([batch["text_ids"]] + [batch[f"false_text_{i}_ids"] for i in range(Fn)], dim=1).reshape(B * (Fn + 1), -1)
    msk = torch.stack([batch["text_masks"]] + [batch[f"false_text_{i}_masks"] for i in range(Fn)], dim=1).reshape(B * (Fn + 1), -1)
    imgs = img.unsqueeze(1).expand(B, Fn + 1, *img.shape[1:]).reshape(B * (Fn + 1), *img.shape[1:])
    cls = O.infer(p, cfg, ids, msk, imgs)["cls_feats"]
    score = rank_output(p, cls, w, b).view(B, Fn + 1)
    return {"irtr_loss": F.cross_entropy(score, torch.zeros(B, dtype=torch.long)), "irtr_scores": score}


def two_steps(p, cfg, batches, labels, lr=LR, wd=WD):
    """Two itm + irtr optimizer steps with the alias semantics of vilt_module.py:233-239: the ITM head is frozen (the ITM loss gives it no
    gradient), rank_output's weight / bias are row 1 of it and take the base learning rate (weight decayed, bias not).  Returns after
    every step (itm_score.fc.weight, itm_score.fc.bias, losses)."""
    p = {n: t.clone() for n, t in p.items() if not n.startswith(("k_", "moco_head"))}
    frozen = ("itm_score.fc.weight", "itm_score.fc.bias")
    m = {n: torch.zeros_like(t) for n, t in p.items()}
    v = {n: torch.zeros_like(t) for n, t in p.items()}
    out = []
    for step, (batch, lab) in enumerate(zip(batches, labels), 1):
        q = {n: (t.clone().requires_grad_(n not in frozen)) for n, t in p.items()}
        rw = p["itm_score.fc.weight"][1:].clone().requires_grad_(True)
        rb = p["itm_score.fc.bias"][1:].clone().requires_grad_(True)
        itm = O.compute_itm_wpa(q, cfg, batch, lab)
        irtr = compute_irtr(q, cfg, batch, rw, rb)
        (itm["itm_loss"] + itm["itm_wpa_loss"] + irtr["irtr_loss"]).backward()
        for n, t in p.items():
            if n in frozen or q[n].grad is None:
                continue
            decay, _ = O.param_group(n)
            O.adamw_step(t, q[n].grad, m[n], v[n], step, lr, wd if decay else 0.0)
        w1, b1 = p["itm_score.fc.weight"][1:], p["itm_score.fc.bias"][1:]                   # views: the step moves the ITM head's row 1
        O.adamw_step(w1, rw.grad, m["itm_score.fc.weight"][1:], v["itm_score.fc.weight"][1:], step, lr, wd)
        O.adamw_step(b1, rb.grad, m["itm_score.fc.bias"][1:], v["itm_score.fc.bias"][1:], step, lr, 0.0)
        out.append((p["itm_score.fc.weight"].clone(), p["itm_score.fc.bias"].clone(),
                    {"itm_loss": float(itm["itm_loss"]), "itm_wpa_loss": float(itm["itm_wpa_loss"]), "irtr_loss": float(irtr["irtr_loss"])}))
    return out


# ---- recall ---------------------------------------------------------------------------------------------------------------------------
def visual_embed(p, cfg, img, select=None):
    """VisionTransformer.visual_embed for one zero-padded batch, WITHOUT the token-type row: (embeds, masks, select or None)."""
    S = cfg["image_size"]
    if img.shape[2] == S and img.shape[3] == S and select is None and bool((O.patch_mask(img, cfg["patch_size"]) == 1).all()):
        ie, im = O.visual_embed_dense(p, "", img, cfg)
        return ie, im, None
    return O.visual_embed(p, "", img, cfg, select)


def infer_embeds(p, cfg, ids, masks, ie, im) -> torch.Tensor:
    """cls_feats of infer(batch, image_embeds=ie, image_masks=im) (vilt_module.py:296-351)."""
    te = O.text_embed(p, "", ids) + p["token_type_embeddings.weight"][0]
    x = torch.cat([te, ie + p["token_type_embeddings.weight"][1]], dim=1)
    m = torch.cat([masks, im], dim=1)
    for i in range(cfg["num_layers"]):
        x = O.block(p, f"transformer.blocks.{i}.", x, m, cfg["num_heads"])
    x = O.layer_norm(x, p["transformer.norm.weight"], p["transformer.norm.bias"], 1e-6)
    return torch.tanh(x[:, 0] @ p["pooler.dense.weight"].t() + p["pooler.dense.bias"])


def recall_from_scores(scores, iids, tiids):
    """R@k of objectives.py:1318-1344, restated: a row (image) counts for text retrieval when one of its k best captions is its own, a
    column (caption) for image retrieval when its image is among its k best.  Returns (ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10)."""
    own = iids.view(-1, 1) == tiids.view(1, -1)
    tr = [own.gather(1, scores.topk(k, dim=1).indices).any(dim=1).float().sum() / own.shape[0] for k in (1, 5, 10)]
    ir = [own.gather(0, scores.topk(k, dim=0).indices).any(dim=0).float().sum() / own.shape[1] for k in (1, 5, 10)]
    return (*ir, *tr)


def score_matrix(p, cfg, images, selects, text_ids, text_masks) -> torch.Tensor:
    rows = []
    for img, sel in zip(images, selects):
        ie, im, _ = visual_embed(p, cfg, img, sel)
        n = text_ids.shape[0]
        cls = infer_embeds(p, cfg, text_ids, text_masks, ie.expand(n, -1, -1), im.expand(n, -1))
        rows.append(rank_output(p, cls))
    return torch.stack(rows)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
# name -> (B, F, layers, weight seed, batch seed, image sizes or None)
CASES = {
    "irtr_L2_B2_F3": (2, 3, 2, 21, 41, None),
    "irtr_L12_B2_F15": (2, 15, 12, 22, 42, None),
    "irtr_L2_B3_F2_raggedimg": (3, 2, 2, 23, 43, [(384, 320), (256, 384), (320, 352)]),
}
FIXTURES = tuple(CASES)
TWO_STEP = "irtr2_L2_B2_F3"
RECALL = "irtr_recall_L2"
# eleven images of five sizes x fifteen captions whose image index repeats: every row and column has an 11th score, so the decision
# boundary of R@10 exists in both directions (and the reference's scores.topk(10, dim=0) needs >= 10 images)
RECALL_SIZES = [(384, 384), (320, 384), (384, 320), (256, 352), (384, 384), (320, 384), (384, 320), (384, 384), (256, 352), (320, 384),
                (352, 352)]
RECALL_TIIDS = [0, 0, 1, 2, 2, 2, 3, 5, 5, 6, 7, 7, 9, 10, 10]
TOL_SCORE_F32 = 2e-3                       # the fp32 score class of tests/test_nlvr2_gpu.py TOL (relative to max(1, max |score|))


def _cfg(layers, B, Fn):
    cfg = O.default_config(num_layers=layers, num_negative=1024, per_gpu_batchsize=B)
    cfg["draw_false_text"] = Fn
    return cfg


def case_inputs(name: str):
    """(cfg, params, batch) of a single-step fixture."""
    B, Fn, layers, sw, sb, sizes = CASES[name]
    cfg = _cfg(layers, B, Fn)
    return cfg, O.init_params(cfg, sw), irtr_batch(cfg, B, Fn, sb, sizes)


def two_step_inputs():
    """(cfg, params, [batch 1, batch 2]) of the two-step fixture (the ITM labels of each step are recorded in the fixture)."""
    cfg = _cfg(2, 2, 3)
    return cfg, O.init_params(cfg, 24), [irtr_batch(cfg, 2, 3, 44), irtr_batch(cfg, 2, 3, 45)]


def recall_inputs(draw: bool = True):
    """(cfg, params, images (one [1, 3, H, W] each, at its own size), iids, text ids, masks, tiids).  draw: rank_output's row and bias are
    the ones the generator drew and stored in the fixture (tools/gen_golden_irtr.py: scores with clear decision boundaries)."""
    cfg = _cfg(2, 1, 0)
    p = O.init_params(cfg, 25)
    if draw:
        g = load(RECALL)
        p["itm_score.fc.weight"][1] = torch.from_numpy(g["rank_w"])
        p["itm_score.fc.bias"][1] = float(g["rank_b"])
    images = []
    for i, (h, w) in enumerate(RECALL_SIZES):
        gen = torch.Generator().manual_seed(500 + i)
        images.append(torch.rand(1, 3, h, w, generator=gen) * 2 - 1)
    ids, masks, _ = synthetic_text(cfg, len(RECALL_TIIDS), 46)
    return cfg, p, images, list(range(len(images))), ids, masks, torch.tensor(RECALL_TIIDS)


def adam_movement(grads, lr=LR, b1=0.9, b2=0.98, eps=1e-8, torch_form=False):
    """sum of the first len(grads) Adam updates (bias-corrected, no decay) of elements whose gradients were grads[0], grads[1], ...
    transformers.AdamW (what the reference trains with and FusedAdamW restates) adds eps to sqrt(v) BEFORE the bias correction,
    torch.optim.AdamW (torch_form, what wrote the two-step fixture) after it: they differ for gradients of eps' own size."""
    import numpy as np
    m = v = total = np.zeros_like(np.asarray(grads[0], dtype=np.float64))
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, dtype=np.float64)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        if torch_form:
            total = total - lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
        else:
            total = total - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(v) + eps)
    return total


def check_adam_row(got, ref, init, grads, what, lr=LR, wd=WD, cls=2e-3, grad_floor=0.0):
    """A parameter row after len(grads) AdamW steps against the reference's, with NO tolerance of its own: the only input is the
    repository's fp32 gradient class (`cls` = 2e-3 of the largest entry, tests/test_nlvr2_gpu.py TOL).  grads are the REFERENCE's
    gradients of the row at every step (stored in the fixture).  Adam's update is m / (sqrt(v) + eps): for an element whose gradient is
    large against the class it is insensitive to a gradient error (the first step is lr * sign(g) exactly), for one whose gradient
    lies within the class of zero it can be anything inside +-lr per step.  So every element is allowed exactly what gradients INSIDE
    the class can reach: the largest change of adam_movement when every step's gradient moves by -d, 0 or +d (d = cls * max |g| of that
    step), plus the distance between the two AdamW forms (adam_movement), the class itself on the movement (cls * lr per step) and the
    decay term's size (lr * wd * |w| per step).  grad_floor: the rounding floor of a gradient that is analytically zero (the rank bias:
    softmax - onehot sums to 0, what is left is the fp32 rounding of (F + 1) terms of size <= 1 / B per image, (F + 1) * 2^-23)."""
    import itertools
    import numpy as np
    got, ref, init = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, init))
    grads = [np.asarray(g, dtype=np.float64).reshape(-1) for g in grads]
    steps = len(grads)
    base = adam_movement(grads, lr)
    slack = steps * (cls * lr + lr * wd * np.abs(init).max())
    assert float(np.abs(ref - init).max()) > 0.5 * lr, (what, "the reference row did not move")
    assert float(np.abs((ref - init) - adam_movement(grads, lr, torch_form=True)).max()) <= slack, (what, "the fixture does not follow torch's AdamW")
    d = [max(cls * np.abs(g).max(), grad_floor) for g in grads]
    reach = np.zeros_like(base)
    for signs in itertools.product((-1.0, 0.0, 1.0), repeat=steps):
        reach = np.maximum(reach, np.abs(adam_movement([g + sg * dd for g, sg, dd in zip(grads, signs, d)], lr) - base))
    reach = reach + np.abs(base - adam_movement(grads, lr, torch_form=True))     # (triangle: got - ref = (got - base) + (base - ref))
    err = np.abs(got - ref)
    worst = int(np.argmax(err - reach))
    assert np.all(err <= reach + slack), (what, worst, float(err[worst]), float(reach[worst]), slack)
    return float((reach > 0.5 * lr).mean())                              # share of elements the class leaves undetermined (for the log)


def load(name: str):
    from tests.golden_util import load as _load
    return _load(name + ".npz")
