"""Generate the masked-patch-prediction golden fixtures tests/golden/mpp_*.npz and mlm_itm_mpp_L2_B4.npz by running the REFERENCE's own
compute_mpp (vilt/modules/objectives.py:632-665) - and compute_mlm + compute_itm_wpa for the combined case - on the reference's own
heads.MPPHead(bert_config) and VisionTransformer.mask_tokens.

TEST INFRASTRUCTURE ONLY: runs on the build machine only (needs the reference checkout that oracle/gen_golden.py imports).  It imports
oracle.gen_golden (its stand-ins, Holder - whose infer(**kw) forwards mask_image -, tensor_digest) and oracle.rmcl_oracle unchanged; the
head weights, the batches and the pinned masks come from tests/mpp_oracle.py (seeded).

torch.bernoulli is wrapped while the reference runs: the wrapper records the two outputs mask_tokens sees (masked, then the 80 % draw)
and, for the fixtures with pinned edge cases ("ragged", "empty"), hands the seeded masks of mpp_oracle.make_masks to the reference in
their place; for the others the reference's own draw under torch.manual_seed is recorded.  Both are stored in the fixture.

Every fixture is checked here, on the CPU, for near ties: no labelled (row, channel) pair of the reference may have a top-two logit gap
below the bf16 logits tolerance (0.1 x max(1, |z|max)) - the GPU test's exemption for such pairs then cannot hide a wrong argmax.

Usage:  python tools/gen_golden_mpp.py      (writes tests/golden/mpp_*.npz and mlm_itm_mpp_L2_B4.npz, a few minutes)
"""
from __future__ import annotations

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
from tests import mpp_oracle as M  # noqa: E402
from tools.gen_golden_mlm import _accuracy, make_holder as make_mlm_holder  # noqa: E402

NEAR_TIE = 0.1          # the bf16 logits tolerance of tests/test_mpp_gpu.py


class BernoulliTap:
    """torch.bernoulli while the reference runs: records every output; `inject` (a list of float tensors) replaces the draws in order"""

    def __init__(self, inject=None):
        self.inject = list(inject or [])
        self.seen = []
        self.real = torch.bernoulli

    def __call__(self, t, *a, **k):
        out = self.inject.pop(0).to(t.dtype) if self.inject else self.real(t, *a, **k)
        assert out.shape == t.shape
        self.seen.append(out.clone())
        return out

    def __enter__(self):
        torch.bernoulli = self
        return self

    def __exit__(self, *exc):
        torch.bernoulli = self.real


def make_holder(cfg):
    h = make_mlm_holder(cfg)
    bc = G.BertConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_layers"],
                      num_attention_heads=cfg["num_heads"], intermediate_size=cfg["hidden_size"] * cfg["mlp_ratio"],
                      max_position_embeddings=cfg["max_text_len"], hidden_dropout_prob=cfg["drop_rate"],
                      attention_probs_dropout_prob=cfg["drop_rate"])
    h.mpp_score = G.heads.MPPHead(bc)
    # the reference's VisionTransformer.__init__ never creates the `mask_token` its mask_tokens reads (vision_transformer.py:555 would
    # raise an AttributeError): the attribute is supplied here as a parameter of the reference's own module - [1, 1, D] zeros, the shape
    # and start value `feats[indices_replaced] = self.mask_token.to(feats)` implies - and everything else is the reference's arithmetic
    h.transformer.mask_token = torch.nn.Parameter(torch.zeros(1, 1, cfg["hidden_size"]))
    for phase in ("train", "val"):
        setattr(h, f"{phase}_mpp_loss", lambda x: x)
        setattr(h, f"{phase}_mpp_accuracy", _accuracy)
    return h


def run_mpp(tag, B, seed_w, seed_h, seed_b, seed_m, ragged, L, mode, with_mlm_itm, seed_mlm_h=0, seed_mlm=0):
    torch.manual_seed(999)
    cfg, p, batch = M.make_case(B, seed_w, seed_h, seed_b, seed_m, ragged, L, mode, with_mlm_itm, seed_mlm_h, seed_mlm)
    h = make_holder(cfg)
    if not with_mlm_itm:
        del h.mlm_score
    h.load_oracle_params(p)
    h.train()
    img = batch["image"][0]
    inject = None
    if mode in ("ragged", "empty"):
        mk, rp = M.make_masks(img, cfg, seed_m, mode)
        inject = [mk.float(), rp.float()]                                # (the reference ANDs the second draw with the first itself)
    h.zero_grad()
    out = {}
    loss = 0.0
    if with_mlm_itm:
        r1 = G.objectives.compute_mlm(h, deepcopy(batch))
        loss = loss + r1["mlm_loss"]
        out.update(mlm_loss=np.float64(r1["mlm_loss"].item()))
    torch.manual_seed(1000 + seed_m)
    seen_index = []
    plain_infer = h.infer

    def infer_tap(b, **kw):
        r_ = plain_infer(b, **kw)
        seen_index.append(r_["patch_index"])
        return r_

    h.infer = infer_tap
    with BernoulliTap(inject) as tap:
        ret = G.objectives.compute_mpp(h, deepcopy(batch))
    h.infer = plain_infer
    assert len(tap.seen) == 2, len(tap.seen)
    masked, rdraw = tap.seen[0].bool(), tap.seen[1].bool()
    # the reference's slot order: valid patches row-major, EXCEPT that a sample with as many valid patches as the image length gets a
    # random permutation of them (vision_transformer.py:634-636).  The encoder is permutation-equivariant, so the fixture records the
    # per-row quantities in the row-major slot order of this package (ascending flat patch index) and keeps the reference's draw apart.
    (pi, (gh, gw)), = seen_index
    ref_select = (pi[..., 0] * gw + pi[..., 1]).long()
    loss = loss + ret["mpp_loss"]
    if with_mlm_itm:
        r2 = G.objectives.compute_itm_wpa(h, deepcopy(batch))
        loss = loss + r2["itm_loss"] + r2["itm_wpa_loss"]
        out.update(itm_loss=np.float64(r2["itm_loss"].item()), itm_wpa_loss=np.float64(r2["itm_wpa_loss"].item()),
                   itm_labels=r2["itm_labels"].numpy())
    out["total_loss"] = np.float64(loss.item())
    n_lab = int((ret["mpp_labels"] != -100).sum())
    if n_lab:
        loss.backward()
    labels = ret["mpp_labels"]                                           # [B, 1 + P, 3]
    logits = ret["mpp_logits"].detach()                                  # [B, 1 + P, 3, 256]
    assert logits.shape == tuple(labels.shape) + (256,)
    # the oracle restates the reference: labels equal, loss to fp32 rounding
    assert torch.equal(labels, M.image_labels(img, cfg, masked, select=ref_select)), tag
    with torch.no_grad():
        r = M.compute_mpp(p, cfg, batch, masked, rdraw & masked)
    assert n_lab == 0 or abs(float(r["mpp_loss"]) - float(ret["mpp_loss"])) < 1e-5 * float(ret["mpp_loss"]), (tag, float(r["mpp_loss"]), float(ret["mpp_loss"]))
    on = (labels != -100).any(-1)
    n = int(on.sum())
    bb, tt = on.nonzero(as_tuple=True)
    order = torch.argsort(bb * 100000 + ref_select[bb, tt - 1]) if n else torch.zeros(0, dtype=torch.int64)      # (b, flat patch) ascending
    rows = logits[on].reshape(n, 768)[order]
    lab = labels[on][order]
    canon = M.image_labels(img, cfg, masked)
    assert torch.equal(canon[(canon != -100).any(-1)], lab), tag
    zg = rows.reshape(n, 3, 256)
    top2 = zg.topk(2, dim=2).values if n else torch.zeros(0, 3, 2)
    gap = top2[..., 0] - top2[..., 1]
    zmax = float(rows.abs().max()) if n else 0.0
    assert n == 0 or float(gap.min()) >= NEAR_TIE * max(1.0, zmax), (tag, float(gap.min()), zmax)      # no near-tie pair: re-seed if this fires
    argmax = zg.argmax(dim=2) if n else torch.zeros(0, 3, dtype=torch.int64)
    out.update(mpp_loss=np.float64(ret["mpp_loss"].item()), n=np.int64(n), correct=np.int64(int((argmax == lab).sum())),
               log_accuracy=np.float64(h.logged["mpp/train/accuracy"]), log_loss=np.float64(h.logged["mpp/train/loss"]),
               image_labels=canon.numpy(), image_labels_ref=labels.numpy(), ref_select=ref_select.numpy(), masked=masked.numpy(), replaced_draw=rdraw.numpy(), argmax=argmax.numpy(), gap=gap.numpy(),
               zmax=np.float64(zmax), row_logits=rows.numpy(), labels=lab.numpy(),
               row_loss=torch.nn.functional.cross_entropy(zg.reshape(-1, 256), lab.reshape(-1), reduction="none").reshape(n, 3).numpy()
               if n else np.zeros((0, 3), np.float32))
    gnames, gd = [], []
    for name, prm in h.named_parameters():
        if not name.startswith("k_") and prm.grad is not None:
            gnames.append(name)
            gd.append(G.tensor_digest(prm.grad))
    out["grad_names"] = np.array(gnames)
    out["grad_digest"] = np.stack(gd) if gd else np.zeros((0, 11))
    if n:
        ms = h.mpp_score
        out["grad_mask_token"] = h.transformer.mask_token.grad.flatten().numpy().copy()
        out["grad_decoder_w"] = ms.decoder.weight.grad[::48, :64].numpy().copy()
        out["grad_decoder_b"] = ms.decoder.bias.grad.numpy().copy()
        out["grad_dense_w"] = ms.transform.dense.weight.grad[:8, :64].numpy().copy()
        out["grad_patch_w"] = h.transformer.patch_embed.proj.weight.grad.reshape(768, -1)[:8, :64].numpy().copy()
        out["grad_patch_b"] = h.transformer.patch_embed.proj.bias.grad.numpy().copy()
    out["meta"] = np.array([B, seed_w, seed_h, seed_b, seed_m, int(ragged), L, M.MODES.index(mode), int(with_mlm_itm), seed_mlm_h, seed_mlm],
                           dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", f"{tag}.npz")
    golden_util.save(path, out)
    print(os.path.basename(path), "loss", out["mpp_loss"], "n", n, "correct", int(out["correct"]), "min gap", float(gap.min()) if n else None,
          "zmax", zmax, "masked", int(masked.sum()), "replaced", int((rdraw & masked).sum()), "bytes", os.path.getsize(path))


CASES = (("mpp_L2_B4_ragged", 4, 11, 171, 121, 181, True, 2, "ragged", False),
         ("mpp_L2_B2_empty", 2, 11, 173, 124, 183, False, 2, "empty", False),
         ("mlm_itm_mpp_L2_B4", 4, 11, 172, 123, 182, True, 2, "random", True, 72, 82),
         ("mpp_L12_B2", 2, 12, 174, 122, 184, False, 12, "random", False))

if __name__ == "__main__":
    torch.set_num_threads(16)
    only = set(sys.argv[1:])                                             # fixture names: regenerate those alone
    for case in CASES:
        if not only or case[0] in only:
            run_mpp(*case)
