"""Generate the alignment fixture tests/golden/align_L2.npz by running the REFERENCE's own model (its BertEmbeddings, VisionTransformer,
Pooler through oracle.gen_golden.Holder), its cost_matrix_cosine and ipot (vilt/modules/objectives.py) and the heat arithmetic of its demo
(demo.py:129-148) on the toy vocabulary, L = 2 layers: one square image and one ragged pair (tests/align_fixture.py).

TEST INFRASTRUCTURE ONLY: runs on the build machine only, on the CPU (needs the reference checkout that oracle/gen_golden.py imports).  It
imports oracle.gen_golden and oracle.rmcl_oracle unchanged.  The heat arithmetic of the demo is nested inside its main() and cannot be
imported; demo_heat below restates it line by line in torch float32.

The reference returns the image tokens of a sample in a random order (vision_transformer.py:633-636); they are put back in row-major
order of their patches before the cost is formed - the order the engine keeps - which permutes the plan's rows and nothing else.

Stored per case: ids, masks, the patch cell of every image slot (-1: a padding slot), the reference's text_feats / image_feats, the
demo's masks, cost, the plan at 50 and at 1000 iterations with e32 = max |ipot(fp32) - ipot(fp64)| on that cost (the base of the
kernel allowance of tests/test_wpa_kernels_gpu.py), the heat maps and bytes of every text position, the bytes that are stable under the
margin (tests/align_fixture.py), one chosen position per sample and its alpha channel as PIL's NEAREST resize makes it.

Margin condition: no test may skip a decision, so the generator refuses a seed in which the non-zero set or the arg-max of a recorded map
changes under a relative perturbation of 4 t DC_BUDGET / beta (tests/align_fixture.py).

Usage:  python tools/gen_golden_align.py      (writes tests/golden/align_L2.npz, under a minute)
"""
from __future__ import annotations

import os
import sys
from copy import deepcopy

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins, imports the reference)
from oracle import rmcl_oracle as O  # noqa: E402
from tests import align_fixture as AF  # noqa: E402
from tests import align_ref as R  # noqa: E402
from tests import golden_util  # noqa: E402


def demo_heat(plan_b, hidx, cells, H, W, n_batch):
    """demo.py:129-146 for text position hidx of one sample: plan_b [Li, Lt] fp32, cells = the (h, w) of every image slot behind cls.
    Returns (heat [H, W] fp32 - NaN where the demo divides by zero, bytes uint8 [H, W])"""
    cost_ = (plan_b * n_batch).t()[hidx][1:]
    heatmap = torch.zeros(H, W)
    for i, (h, w) in enumerate(cells):
        if h >= 0:
            heatmap[h, w] = cost_[i]
    heatmap = (heatmap - heatmap.mean()) / heatmap.std()
    heatmap = torch.clamp(heatmap, 1.0, 3.0)
    heatmap = (heatmap - heatmap.min()) / (heatmap.max() - heatmap.min())
    with np.errstate(invalid="ignore"):
        return heatmap, np.uint8(np.nan_to_num(heatmap.numpy()) * 255)


def run_case(case, out):
    cfg = AF.config()
    c = AF.CASES[case]
    B = c["B"]
    batch = AF.make_batch(cfg, case)
    p = O.init_params(cfg, AF.SEEDS["weights"])
    h = G.Holder(cfg)
    h.load_oracle_params(p)
    h.eval()
    torch.manual_seed(4321)
    with torch.no_grad():
        r = h.infer(deepcopy(batch))
    pi, (H, W) = r["patch_index"]
    H, W = int(H), int(W)
    flat = (pi[..., 0] * W + pi[..., 1]).clone()
    img_f, msk = r["image_feats"].clone(), r["image_masks"]
    for b in range(B):                                         # valid tokens back in row-major order; padding slots get cell -1
        nv = int(msk[b, 1:].sum())
        order = torch.argsort(flat[b, :nv])
        img_f[b, 1:1 + nv] = img_f[b, 1:1 + nv][order]
        flat[b, :nv] = flat[b, :nv][order]
        flat[b, nv:] = -1
        assert bool(msk[b, 1:1 + nv].all()) and not bool(msk[b, 1 + nv:].any())
    txt_f = r["text_feats"]
    txt_mask, img_mask = AF.demo_masks(r["text_masks"], msk)
    txt_pad, img_pad = ~txt_mask, ~img_mask
    with torch.no_grad():
        cost = G.objectives.cost_matrix_cosine(txt_f.float(), img_f.float())
    joint_pad = txt_pad.unsqueeze(-1) | img_pad.unsqueeze(-2)
    cost.masked_fill_(joint_pad, 0)
    txt_len = (txt_pad.size(1) - txt_pad.sum(dim=1)).to(cost.dtype)
    img_len = (img_pad.size(1) - img_pad.sum(dim=1)).to(cost.dtype)
    Lt = txt_f.shape[1]
    cells = [[(int(f) // W, int(f) % W) if f >= 0 else (-1, -1) for f in flat[b]] for b in range(B)]
    out.update({f"{case}_ids": batch["text_ids"].numpy(), f"{case}_masks": batch["text_masks"].numpy(), f"{case}_cells": flat.numpy().astype(np.int32),
                f"{case}_grid_hw": np.array([H, W]), f"{case}_text_feats": txt_f.numpy(), f"{case}_image_feats": img_f.numpy(),
                f"{case}_txt_valid": txt_mask.numpy(), f"{case}_img_valid": img_mask.numpy(), f"{case}_cost": cost.numpy()})
    token = None
    for t in AF.ITERS:
        T = G.objectives.ipot(cost.detach(), txt_len, txt_pad, img_len, img_pad, joint_pad, AF.BETA, t, 1)
        T64 = O.ipot(cost.double(), txt_len.double(), txt_pad, img_len.double(), img_pad, joint_pad, AF.BETA, t, 1)
        e32 = float((T.double() - T64).abs().max())
        heat = np.zeros((B, Lt, H, W), dtype=np.float32)
        by = np.zeros((B, Lt, H, W), dtype=np.uint8)
        flat_ref = np.zeros((B, Lt), dtype=np.int32)
        byte_ok = np.zeros((B, Lt, H, W), dtype=bool)
        grid64 = R.scatter(T.double().numpy(), flat.numpy(), H, W)
        rel = AF.relative_bound(t, AF.DC_BUDGET)
        for b in range(B):
            for m in range(Lt):
                hm, bm = demo_heat(T[b], m, cells[b], H, W, B)
                if bool(torch.isnan(hm).any()):
                    flat_ref[b, m] = 1
                    continue
                heat[b, m], by[b, m] = hm.numpy(), bm
                assert bool(txt_mask[b, m]), (case, t, b, m)                    # only a masked position may be NaN-free by accident
                stable, ok = AF.stability(grid64[b, m], rel, seed=1000 * t + 100 * b + m)
                assert stable, ("re-seed tests/align_fixture.SEEDS", case, t, b, m)
                byte_ok[b, m] = ok
        model_flat = R.heat_model(grid64, txt_mask.numpy())[1]
        assert np.array_equal(model_flat, flat_ref), (case, t)                    # the demo is NaN exactly where the model says flat
        live = [[m for m in range(Lt) if not flat_ref[b, m]] for b in range(B)]
        assert all(live), (case, t, "a sample without a non-flat position")
        out.update({f"{case}_plan_{t}": T.numpy(), f"{case}_e32_{t}": np.array([e32, float(T64.max())]), f"{case}_heat_{t}": heat,
                    f"{case}_bytes_{t}": by, f"{case}_byte_ok_{t}": byte_ok, f"{case}_flat_{t}": flat_ref})
        print(case, "t", t, "e32 %.3e max T %.3e" % (e32, float(T64.max())), "flat", int(flat_ref.sum()), "of", flat_ref.size,
              "stable bytes", int(byte_ok.sum()), "of", int((1 - flat_ref).sum()) * H * W, "relative bound %.3g" % rel)
        if t == AF.ITERS[-1]:
            token = [live[b][len(live[b]) // 2] for b in range(B)]
            Hp, Wp = batch["image"][0].shape[2:]
            alpha = np.stack([np.array(Image.fromarray(by[b, token[b]], "L").resize((Wp, Hp), resample=Image.NEAREST)) for b in range(B)])
            out.update({f"{case}_token": np.array(token, dtype=np.int64), f"{case}_alpha_{t}": alpha})


if __name__ == "__main__":
    torch.set_num_threads(16)
    out = {"meta": np.array([AF.SEEDS["weights"], AF.SEEDS["batch"]], dtype=np.int64)}
    for case in AF.CASES:
        run_case(case, out)
    path = os.path.join(ROOT, "tests", "golden", AF.FIXTURE)
    golden_util.save(path, out)
    print(os.path.basename(path), "bytes", os.path.getsize(path))
