"""CPU oracle of the masked-patch-prediction step (test infrastructure): the reference's VisionTransformer.mask_tokens
(vision_transformer.py:525-557) with the masks GIVEN instead of drawn, visual_embed(mask_it=True) (:559-677), MPPHead (heads.py:198-207),
compute_mpp's cross-entropy (objectives.py:632-665) and its Accuracy metric (gadgets/my_metrics.py:5-28), restated in torch on top of
oracle.rmcl_oracle.  Also the seeded head weights and the seeded mask maker, so a case is reproducible from (cfg, seeds): the head's
weights are never stored."""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from oracle import rmcl_oracle as O

MODES = ("random", "ragged", "empty")


def mpp_param_shapes(cfg: dict) -> List[Tuple[str, Tuple[int, ...]]]:
    """transformer.mask_token and MPPHead(bert_config): BertPredictionHeadTransform + Linear(D, 768) with bias."""
    D = cfg["hidden_size"]
    return [("transformer.mask_token", (1, 1, D)), ("mpp_score.transform.dense.weight", (D, D)), ("mpp_score.transform.dense.bias", (D,)),
            ("mpp_score.transform.LayerNorm.weight", (D,)), ("mpp_score.transform.LayerNorm.bias", (D,)),
            ("mpp_score.decoder.weight", (768, D)), ("mpp_score.decoder.bias", (768,))]


HEAD = [n for n, _ in mpp_param_shapes({"hidden_size": 768})]


def mpp_init_params(cfg: dict, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded weights: N(0, 0.02) matrices like the reference's init_weights, with non-trivial biases, LayerNorm affine terms and mask
    token so that their gradients are exercised off the init point.  One class per channel gets a raised output bias (6) and another a
    smaller one (2): random 0.02-scale logits over 256 classes have top-two gaps far below the bf16 logits tolerance, a fixture with a
    DECIDED argmax needs structure."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in mpp_param_shapes(cfg):
        if name.endswith("LayerNorm.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t.float()
    for c, (a, b) in enumerate(dominant_classes(seed)):
        out["mpp_score.decoder.bias"][256 * c + a] = 6.0
        out["mpp_score.decoder.bias"][256 * c + b] = 2.0
    return out


def dominant_classes(seed: int):
    """(raised, second) class per channel.  The patch means of uniform pixels sit at 127.5 +- 2.3, so the raised classes are taken from
    126..129: some labelled pairs are then predicted correctly and the accuracy of a fixture is not trivially zero."""
    g = torch.Generator().manual_seed(seed + 7919)
    out = []
    for _ in range(3):
        t = (torch.randperm(4, generator=g)[:2] + 126).tolist()
        out.append((t[0], t[1]))
    return out


def patch_labels(img: torch.Tensor, ps: int = 32) -> torch.Tensor:
    """mask_tokens' labels over the FULL grid (vision_transformer.py:529-544): the fp32 grouped conv2d with weights 1 / (ps ps) of
    img * 0.5 + 0.5, times 255, truncated.  [B, G, 3] int64."""
    u = img.float() * 0.5 + 0.5
    m = F.conv2d(u, weight=torch.ones(3, 1, ps, ps) / (ps * ps), bias=None, stride=(ps, ps), padding=0, groups=3)
    return (m * 255).long().flatten(start_dim=2, end_dim=3).permute(0, 2, 1).contiguous()


def patch_means_fp64(img: torch.Tensor, ps: int = 32) -> torch.Tensor:
    """the same quantity before truncation, in fp64: [B, G, 3]"""
    u = img.double() * 0.5 + 0.5
    B, C, H, W = u.shape
    m = u.reshape(B, C, H // ps, ps, W // ps, ps).mean(dim=(3, 5))
    return (m * 255).flatten(start_dim=2, end_dim=3).permute(0, 2, 1).contiguous()


def selection(img: torch.Tensor, cfg: dict, select=None):
    """(sel [B, n] flat patch indices, valid [B, n] bool) of the batch: the whole grid for full-size images, else O.ragged_select."""
    ps, S = cfg["patch_size"], cfg["image_size"]
    B = img.shape[0]
    if img.shape[2] == S and img.shape[3] == S and select is None and bool((O.patch_mask(img, ps) == 1).all()):
        G = (S // ps) ** 2
        return torch.arange(G).repeat(B, 1), torch.ones(B, G, dtype=torch.bool)
    m, _, _ = O.ragged_geometry(img, ps)
    sel, n = O.ragged_select(m, cfg.get("max_image_len", -1), select)
    return sel, torch.gather(m.flatten(1), 1, sel).bool()


def make_masks(img: torch.Tensor, cfg: dict, seed: int, mode: str = "random", select=None):
    """Seeded (masked, replaced) [B, G] bool over the full grid.  mode "ragged" (B >= 4) pins the edge cases through the batch's
    selection: sample 0 has NO masked patch; sample 1 masks (and replaces) its first and its last valid slot; sample 2 masks one valid patch
    that is masked but NOT replaced; sample 3 keeps its random draw with at least one replaced patch; the first of samples 2, 3, 1 that
    has a pad slot masks that slot's patch (must be ignored).  mode "empty": nothing is masked (n = 0)."""
    assert mode in MODES, mode
    g = torch.Generator().manual_seed(seed)
    B = img.shape[0]
    ps = cfg["patch_size"]
    G = (img.shape[2] // ps) * (img.shape[3] // ps)
    masked = torch.rand(B, G, generator=g) < 0.15
    replaced = (torch.rand(B, G, generator=g) < 0.8) & masked
    if mode == "empty":
        masked[:] = False
        replaced[:] = False
    if mode == "ragged":
        assert B >= 4
        sel, valid = selection(img, cfg, select)
        masked[0] = False
        replaced[0] = False
        v1 = sel[1][valid[1]]
        for q in (int(v1[0]), int(v1[-1])):
            masked[1, q] = True
            replaced[1, q] = True
        v2 = sel[2][valid[2]]
        q = int(v2[len(v2) // 2])
        masked[2, q] = True
        replaced[2, q] = False
        v3 = sel[3][valid[3]]
        masked[3, int(v3[1])] = True
        replaced[3, int(v3[1])] = True
        for b in (2, 3, 1):                                        # the first of these samples that has a pad slot
            if not bool(valid[b].all()):
                q = int(sel[b][~valid[b]][0])                      # a pad slot's patch: masked and replaced, and ignored
                masked[b, q] = True
                replaced[b, q] = True
                break
    return masked, replaced


def image_labels(img: torch.Tensor, cfg: dict, masked: torch.Tensor, select=None) -> torch.Tensor:
    """image_labels [B, 1 + n, 3] of visual_embed(mask_it=True) (vision_transformer.py:549, 653-659)."""
    lab = patch_labels(img, cfg["patch_size"])
    lab[~masked] = -100
    sel, valid = selection(img, cfg, select)
    lab = torch.gather(lab, 1, sel.unsqueeze(-1).expand(-1, -1, 3)).clone()
    lab[~valid] = -100
    return torch.cat([torch.full((img.shape[0], 1, 3), -100, dtype=lab.dtype), lab], dim=1)


def visual_embed_masked(p, img, cfg, replaced, select=None, drop_mask=None):
    """O.visual_embed / O.visual_embed_dense with `feats[replaced] = mask_token` on the patch-projection output (bias included),
    before the position rows (vision_transformer.py:555, 602-603).  Returns (x [B, 1 + n, D], mask [B, 1 + n])."""
    P = cfg["patch_size"]
    G0 = cfg["image_size"] // P
    W = p["transformer.patch_embed.proj.weight"]
    D = W.shape[0]
    B = img.shape[0]
    Gw = img.shape[3] // P
    xp = O.patchify(img, P).to(W.dtype) @ W.reshape(D, -1).t() + p["transformer.patch_embed.proj.bias"]
    xp = torch.where(replaced.unsqueeze(-1), p["transformer.mask_token"].reshape(1, 1, D).to(xp.dtype), xp)
    sel, valid = selection(img, cfg, select)
    if sel.shape[1] == G0 * G0 and img.shape[2] == cfg["image_size"] and img.shape[3] == cfg["image_size"] and bool(valid.all()) and select is None:
        cls = p["transformer.cls_token"].expand(B, -1, -1)
        x = torch.cat([cls, xp], dim=1) + p["transformer.pos_embed"]
        if drop_mask is not None:
            x = x * drop_mask
        return x, torch.ones(B, 1 + G0 * G0, dtype=torch.int64)
    m, xh, xw = O.ragged_geometry(img, P)
    pos_tab = p["transformer.pos_embed"][0, 1:]
    rows = []
    for b in range(B):
        h, w = int(xh[b]), int(xw[b])
        pe = torch.zeros(img.shape[2] // P, Gw, D, dtype=xp.dtype)
        pe[:h, :w] = O.resize_pos_embed(pos_tab, G0, h, w)
        pe = pe.reshape(-1, D)
        rows.append(xp[b, sel[b]] + pe[sel[b]])
    x = torch.stack(rows)
    cls = (p["transformer.cls_token"][0] + p["transformer.pos_embed"][0, :1]).expand(B, -1, -1)
    x = torch.cat([cls, x], dim=1)
    if drop_mask is not None:                              # pos_drop (vision_transformer.py:667)
        x = x * drop_mask
    return x, torch.cat([torch.ones(B, 1, dtype=torch.int64), valid.long()], dim=1)


def infer_masked(p, cfg, ids, text_masks, img, replaced, select=None, drop=None) -> dict:
    """O.infer with the masked visual_embed (infer(mask_image=True), vilt_module.py:275-351)."""
    drop = drop or {}
    te = O.text_embed(p, "", ids)
    if "text" in drop:
        te = te * drop["text"]
    te = te + p["token_type_embeddings.weight"][0]
    ie, im = visual_embed_masked(p, img, cfg, replaced, select, drop.get("image"))
    ie = ie + p["token_type_embeddings.weight"][1]
    x = torch.cat([te, ie], dim=1)
    m = torch.cat([text_masks, im], dim=1)
    for i in range(cfg["num_layers"]):
        x = O.block(p, f"transformer.blocks.{i}.", x, m, cfg["num_heads"], drop.get(i))
    x = O.layer_norm(x, p["transformer.norm.weight"], p["transformer.norm.bias"], 1e-6)
    L = ids.shape[1]
    return {"text_feats": x[:, :L], "image_feats": x[:, L:], "raw_cls_feats": x[:, 0], "image_masks": im}


def mpp_transform(p, x):
    a = x @ p["mpp_score.transform.dense.weight"].t() + p["mpp_score.transform.dense.bias"]
    return O.layer_norm(O.gelu_erf(a), p["mpp_score.transform.LayerNorm.weight"], p["mpp_score.transform.LayerNorm.bias"], 1e-12)


def mpp_head(p, x):
    """MPPHead.forward (heads.py:204-207)"""
    return mpp_transform(p, x) @ p["mpp_score.decoder.weight"].t() + p["mpp_score.decoder.bias"]


def compact(labels: torch.Tensor, L: int):
    """The compaction restated: image_labels [B, 1 + P, 3] -> (row b N + L + t of every labelled image row in ascending order,
    lab [n, 3], n), N = L + 1 + P."""
    B, P1, _ = labels.shape
    N = L + P1
    on = (labels != -100).any(dim=-1)
    b, t = on.nonzero(as_tuple=True)
    return (b * N + L + t), labels[on], int(on.sum())


def compute_mpp(p, cfg, batch, masked, replaced, select=None, drop=None) -> dict:
    """compute_mpp (objectives.py:632-665).  The logits are formed on the labelled rows only (cross_entropy ignores the others)."""
    img = batch["image"][0]
    out = infer_masked(p, cfg, batch["text_ids"], batch["text_masks"], img, replaced, select, drop)
    labels = image_labels(img, cfg, masked, select)
    on = (labels != -100).any(dim=-1)
    z = mpp_head(p, out["image_feats"][on])                         # [n, 768]
    lab = labels[on]                                                # [n, 3]
    zz, ll = z.reshape(-1, 256), lab.reshape(-1)
    loss = F.cross_entropy(zz, ll, reduction="sum") / ll.numel() if ll.numel() else zz.sum() / 0.0
    correct = int((zz.detach().argmax(dim=-1) == ll).sum())
    return {"mpp_loss": loss, "mpp_rows": z, "mpp_labels": labels, "image_feats": out["image_feats"], "correct": correct,
            "pairs": int(ll.numel()), "n": int(on.sum())}


FIXTURES = ("mpp_L2_B4_ragged", "mpp_L12_B2", "mpp_L2_B2_empty", "mlm_itm_mpp_L2_B4")
RAGGED_SIZES = [(384, 352), (320, 384), (384, 384), (224, 288)]     # zero-padded to 384 x 384 (sample 3 leaves pad slots)


def make_case(B, seed_w, seed_h, seed_b, seed_m, ragged, L, mode, with_mlm_itm, seed_mlm_h=0, seed_mlm=0):
    """(cfg, params incl. the heads, batch) of a fixture from its seeds.  `ragged`: ragged text and zero-padded images."""
    cfg = O.default_config(num_layers=L, num_negative=1024 if L == 2 else 65536, per_gpu_batchsize=B)
    p = dict(O.init_params(cfg, seed_w), **mpp_init_params(cfg, seed_h))
    batch = O.synthetic_batch(cfg, B, seed_b, ragged_text=bool(ragged), sizes=RAGGED_SIZES[:B] if ragged else None)
    if with_mlm_itm:
        from tests import mlm_oracle as ML
        p.update(ML.mlm_init_params(cfg, seed_mlm_h))
        batch = ML.synthetic_mlm(batch, seed_mlm, cfg["vocab_size"], "random", dup_label=ML.dominant_tokens(cfg, seed_mlm_h)[0])
    return cfg, p, batch


def load_case(name: str):
    """An mpp fixture with everything needed to recompute it: (fixture, cfg, params, batch, masked, replaced, with_mlm_itm).  The masks are
    the two bernoulli outputs the reference's mask_tokens saw, as recorded (replaced already AND-ed with masked)."""
    from tests.golden_util import load
    g = load(name + ".npz")
    B, sw, sh, sb, sm, ragged, L, mode, with_mlm_itm, smh, sml = [int(x) for x in g["meta"]]
    cfg, p, batch = make_case(B, sw, sh, sb, sm, ragged, L, MODES[mode], bool(with_mlm_itm), smh, sml)
    masked = torch.from_numpy(g["masked"]).bool()
    replaced = torch.from_numpy(g["replaced_draw"]).bool() & masked
    return g, cfg, p, batch, masked, replaced, bool(with_mlm_itm)
