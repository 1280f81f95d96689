"""Generate the image-text retrieval fixtures tests/golden/irtr*.npz / irtr_configs.json by running the REFERENCE's own compute_irtr,
compute_itm_wpa and compute_irtr_recall (vilt/modules/objectives.py:714-787, :1180-1346) with its rank_output alias
(vilt_module.py:233-239: rank_output.weight / .bias are VIEWS of row 1 of itm_score.fc, the ITM head is frozen).

TEST INFRASTRUCTURE ONLY: runs on the build machine only (needs the reference checkout that oracle/gen_golden.py imports).  It imports
oracle.gen_golden (its stand-ins, Holder, tensor_digest) unchanged; weights, batches, images and captions come seeded from
tests/irtr_oracle.py, so every fixture is reproducible.

  irtr_L2_B2_F3, irtr_L12_B2_F15, irtr_L2_B3_F2_raggedimg   one compute_irtr step: loss, [B, F + 1] scores, gradient digests, the log.
  irtr2_L2_B2_F3    TWO itm + irtr steps with torch.optim.AdamW between them (the reference's parameter groups, betas, eps): the ITM
                    head and rank_output after each step - row 1 moves with rank_output, row 0 does not move.
  irtr_recall_L2    compute_irtr_recall on 11 images (five sizes) x 15 captions with stand-ins for trainer.datamodule.dms[0] and a
                    one-process gloo group: the visual_embed outputs with the drawn patch_index, the score matrix, tiids, iids, the six
                    recalls.  (11 images: the reference's scores.topk(10, dim=0) needs 10, and the R@10 boundary an 11th.)  The rank
                    row is FITTED here (run_recall, step 2) so that, on the reference's own scores, the gap at every decision boundary
                    (between the k-th and (k + 1)-th score of every row and column, k = 1, 5, 10) is at least 20 x the fp32 score
                    tolerance and R@10 is not trivial; the row, its bias and the smallest gap are stored in the fixture.
  irtr_configs.json the values of the reference's four task_finetune_irtr_* named configs, read from its config file as data.

Usage:  python tools/gen_golden_irtr.py [fixture names | two_step | recall | configs]
"""
from __future__ import annotations

import ast
import json
import os
import sys
import tempfile
import types
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins, imports the reference)
from tests import golden_util  # noqa: E402
from tests import irtr_oracle as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _holder(cfg, p):
    h = G.Holder(dict(cfg, num_workers=0))
    h.load_oracle_params(p)
    D = cfg["hidden_size"]
    # the alias of an IRTR model: a rank head whose tensors are VIEWS of row 1 of the ITM head, and an ITM head that takes no gradient
    head, rank = h.itm_score.fc, nn.Linear(D, 1)
    rank.weight.data, rank.bias.data = head.weight.data[1:], head.bias.data[1:]
    head.requires_grad_(False)
    h.rank_output = rank
    assert rank.weight.data_ptr() == head.weight[1:].data_ptr() and rank.bias.data_ptr() == head.bias[1:].data_ptr()
    for ph in ("train", "val"):
        setattr(h, f"{ph}_irtr_loss", lambda x: x)
    h.captured = []
    h.rank_output.register_forward_hook(lambda mod, inp, out: h.captured.append((inp[0].detach().clone(), out.detach().clone())))
    return h


def _grads(h, out):
    gnames, gd = [], []
    for n, prm in h.named_parameters():
        if not n.startswith("k_") and prm.grad is not None:
            gnames.append(n)
            gd.append(G.tensor_digest(prm.grad))
    out["grad_names"] = np.array(gnames)
    out["grad_digest"] = np.stack(gd)
    out["grad_rank_w"] = h.rank_output.weight.grad.numpy().copy()
    out["grad_rank_b"] = h.rank_output.bias.grad.numpy().copy()
    out["grad_pooler_w"] = h.pooler.dense.weight.grad[:8, :64].numpy().copy()
    out["grad_qkv0_w"] = h.transformer.blocks[0].attn.qkv.weight.grad[:8, :64].numpy().copy()


def run_step(name):
    torch.manual_seed(777)
    cfg, p, batch = R.case_inputs(name)
    h = _holder(cfg, p)
    h.train()
    h.zero_grad()
    ret = G.objectives.compute_irtr(h, deepcopy(batch))
    ret["irtr_loss"].backward()
    B, Fn = batch["image"][0].shape[0], cfg["draw_false_text"]
    out = {"irtr_loss": np.float64(ret["irtr_loss"].item()), "irtr_scores": h.captured[-1][1][:, 0].view(B, Fn + 1).numpy()}
    for kk, v in h.logged.items():
        out["log_" + kk.replace("/", "__")] = np.float64(v)
    _grads(h, out)
    assert h.itm_score.fc.weight.grad is None and h.itm_score.fc.bias.grad is None
    golden_util.save(os.path.join(GOLD, f"{name}.npz"), out)
    print(name, float(out["irtr_loss"]), out["irtr_scores"].shape)


def run_two_step():
    torch.manual_seed(778)
    cfg, p, batches = R.two_step_inputs()
    h = _holder(cfg, p)
    h.train()
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight", "norm.bias", "norm.weight", "norm1.bias", "norm1.weight", "norm2.bias",
                "norm2.weight"]                                                 # vilt_utils.py:335-345
    named = [(n, q) for n, q in h.named_parameters() if not n.startswith("k_") and q.requires_grad]
    opt = torch.optim.AdamW([{"params": [q for n, q in named if not any(nd in n for nd in no_decay)], "weight_decay": R.WD},
                             {"params": [q for n, q in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}],
                            lr=R.LR, betas=(0.9, 0.98), eps=1e-8)
    out = {"itm_w_init": h.itm_score.fc.weight.detach().numpy().copy(), "itm_b_init": h.itm_score.fc.bias.detach().numpy().copy(),
           "lr": np.float64(R.LR), "wd": np.float64(R.WD)}
    for s, batch in enumerate(batches, 1):
        opt.zero_grad(set_to_none=True)
        r1 = G.objectives.compute_itm_wpa(h, deepcopy(batch))
        r2 = G.objectives.compute_irtr(h, deepcopy(batch))
        (r1["itm_loss"] + r1["itm_wpa_loss"] + r2["irtr_loss"]).backward()
        assert h.itm_score.fc.weight.grad is None
        if s == 1:
            _grads(h, out)
        out[f"s{s}_grad_rank_w"] = h.rank_output.weight.grad.numpy().copy()     # what tests/irtr_oracle.py check_adam_row conditions on
        out[f"s{s}_grad_rank_b"] = h.rank_output.bias.grad.numpy().copy()
        opt.step()
        out[f"s{s}_itm_labels"] = r1["itm_labels"].numpy().copy()
        out[f"s{s}_itm_loss"], out[f"s{s}_itm_wpa_loss"] = np.float64(r1["itm_loss"].item()), np.float64(r1["itm_wpa_loss"].item())
        out[f"s{s}_irtr_loss"] = np.float64(r2["irtr_loss"].item())
        out[f"s{s}_itm_w"] = h.itm_score.fc.weight.detach().numpy().copy()
        out[f"s{s}_itm_b"] = h.itm_score.fc.bias.detach().numpy().copy()
        out[f"s{s}_rank_w"] = h.rank_output.weight.detach().numpy().copy()
        out[f"s{s}_rank_b"] = h.rank_output.bias.detach().numpy().copy()
        out[f"s{s}_pooler_w_digest"] = G.tensor_digest(h.pooler.dense.weight)
        assert np.array_equal(out[f"s{s}_itm_w"][1], out[f"s{s}_rank_w"][0]) and np.array_equal(out[f"s{s}_itm_w"][0], out["itm_w_init"][0])
        assert not np.array_equal(out[f"s{s}_itm_w"][1], out["itm_w_init"][1])
    golden_util.save(os.path.join(GOLD, f"{R.TWO_STEP}.npz"), out)
    print(R.TWO_STEP, {k: float(v) for k, v in out.items() if k.endswith("_loss")})


class _ToyDset(torch.utils.data.Dataset):
    """stand-in for make_no_false_val_dset's dataset: pre-tokenised captions, or one image per entry (image_only)"""

    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def collate(self, batch, mlm_collator=None):
        if "image" in batch[0]:
            assert len(batch) == 1
            return {"image": [batch[0]["image"]], "img_index": [b["img_index"] for b in batch]}
        return {"text_ids": torch.stack([b["text_ids"] for b in batch]), "text_masks": torch.stack([b["text_masks"] for b in batch]),
                "text_labels": torch.stack([b["text_labels"] for b in batch]), "img_index": [b["img_index"] for b in batch]}


def boundary_gaps(scores: torch.Tensor) -> float:
    """the smallest gap between the k-th and (k + 1)-th largest score over every row and column, k = 1, 5, 10 (every row and column must
    hold at least 11 scores)"""
    gaps = []
    for dim in (0, 1):
        s = scores.sort(dim=dim, descending=True).values
        assert s.shape[dim] > 10, tuple(scores.shape)
        for k in (1, 5, 10):
            gaps.append((s.narrow(dim, k - 1, 1) - s.narrow(dim, k, 1)).min())
    return float(torch.stack(gaps).min())


def run_recall():
    import torch.distributed as dist
    torch.manual_seed(779)
    cfg, p, images, iids, ids, masks, tiids = R.recall_inputs(draw=False)
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tempfile.mkdtemp(), "pg"), rank=0, world_size=1)
    labels = torch.full_like(ids, -100)
    texts = [{"text_ids": ids[j], "text_masks": masks[j], "text_labels": labels[j], "img_index": int(tiids[j])} for j in range(len(tiids))]
    imgs = [{"image": images[i], "img_index": iids[i]} for i in range(len(images))]
    dm = types.SimpleNamespace(tokenizer=None, mlm_collator=None,
                               make_no_false_val_dset=lambda image_only=False, max_num=-1: _ToyDset(imgs if image_only else texts))

    def reference_run(pp):
        h = _holder(cfg, pp)
        h.eval()
        h.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(dms=[dm]))
        ve = h.transformer.visual_embed
        seen = []

        def recording(*a, **kw):
            r = ve(*a, **kw)
            seen.append(r)
            return r

        h.transformer.visual_embed = recording
        rec = G.objectives.compute_irtr_recall(h)
        cls = torch.stack([c for c, _ in h.captured])                       # [n_img, n_txt, D]
        sc = torch.stack([s[:, 0] for _, s in h.captured])
        return rec, cls, sc, seen

    # 1. the reference's pooled cls of every (image, caption) pair, with the seeded weights as they are
    _, cls, _, _ = reference_run(p)
    flat = cls.reshape(-1, cls.shape[-1])
    # 2. fit the rank row.  A plain Gaussian row almost never leaves all 78 decision boundaries of an 11 x 15 matrix clear, so the row is
    #    FITTED: a seeded target a_i + b_j whose image levels a and caption levels b are clustered as 1 | 4 | 5 | rest (steps of 1 between the
    #    clusters, i.e. at ranks 1, 5 and 10; 0.25 of spread inside one) is projected on the 30 leading singular directions of the
    #    reference's centred cls matrix - the directions a cls error is NOT amplified in (the row comes out shorter than a Gaussian row of
    #    the same score range).  The bias centres the scores, the scale puts the largest |score| at 4.  The scores themselves are what
    #    the reference computes with that row: they keep the (image, caption) interaction the target does not have.  Seeds are tried until
    #    the gaps clear 20 x the fp32 score tolerance with margin and R@10 is not trivial in either direction.
    flat64 = flat.double()
    mu = flat64.mean(0)
    U, S, Vh = torch.linalg.svd(flat64 - mu, full_matrices=False)
    n_i, n_t, r = cls.shape[0], cls.shape[1], 30
    with_caption = len(set(tiids.tolist())) / n_i

    def clustered(n, gen):
        sizes, v, lvl = [1, 4, 5, n - 10], [], 0.0
        for m in sizes:
            v += [lvl + 0.25 * float(torch.rand(1, generator=gen)) for _ in range(m)]
            lvl -= 1.0
        v = torch.tensor(v, dtype=torch.float64)
        return v[torch.randperm(n, generator=gen)]

    found = None
    for trial in range(200):
        gen = torch.Generator().manual_seed(20_000 + trial)
        t = (clustered(n_i, gen).view(-1, 1) + clustered(n_t, gen).view(1, -1)).reshape(-1)
        c = U[:, :r].T @ (t - t.mean())
        w = Vh[:r].T @ (c / S[:r])
        sc = (flat64 - mu) @ w
        k = 4.0 / float(sc.abs().max())
        w, b = (w * k).float(), float(-(mu @ w) * k)
        sm = (flat @ w + b).view(n_i, n_t)
        rr = [float(x) for x in R.recall_from_scores(sm, torch.tensor(iids), tiids)]
        if boundary_gaps(sm) >= 1.5 * 20 * R.TOL_SCORE_F32 * 4.0 and 0 < rr[2] < 1 and 0 < rr[5] < with_caption and rr[2] != rr[1] and rr[5] != rr[4]:
            found = (trial, w, b)
            break
    assert found is not None, "no rank row with clear decision boundaries: change the inputs (tests/irtr_oracle.py recall_inputs)"
    trial, w, b = found
    p = dict(p)
    p["itm_score.fc.weight"] = p["itm_score.fc.weight"].clone()
    p["itm_score.fc.bias"] = p["itm_score.fc.bias"].clone()
    p["itm_score.fc.weight"][1] = w
    p["itm_score.fc.bias"][1] = b
    # 3. the reference's compute_irtr_recall with that rank row
    rec, cls2, scores, seen = reference_run(p)
    tol = R.TOL_SCORE_F32 * max(1.0, float(scores.abs().max()))
    gap = boundary_gaps(scores)
    assert gap >= 20 * tol, (gap, tol)
    assert scores.shape[0] > 10 and scores.shape[1] > 10                  # an 11th score in every row and column: the k = 10 boundary exists
    assert 0 < float(rec[2]) < 1 and 0 < float(rec[5]) < with_caption, [float(x) for x in rec]      # R@10 depends on the scores
    out = {"rank_w": w.numpy(), "rank_b": np.float32(b), "rank_trial": np.int64(trial), "scores": scores.numpy(), "tiids": tiids.numpy(),
           "iids": np.array(iids), "recalls": np.array([float(x) for x in rec], dtype=np.float64), "min_gap": np.float64(gap),
           "score_tol": np.float64(tol)}
    for i, (ie, im, (pidx, hw), _) in enumerate(seen[-len(images):]):
        out[f"img{i}_embeds_sub"] = ie[0][:, ::16].contiguous().numpy()      # every 16th column (the whole tensor: its digest)
        out[f"img{i}_embeds_digest"] = G.tensor_digest(ie[0])
        out[f"img{i}_masks"] = im[0].numpy()
        out[f"img{i}_patch_index"] = pidx[0].numpy()
        out[f"img{i}_grid"] = np.array(hw)
    out["cls_0"] = cls2[0].numpy()                                         # infer(image_embeds=...) cls_feats of image 0 x every caption
    golden_util.save(os.path.join(GOLD, f"{R.RECALL}.npz"), out)
    print(R.RECALL, "trial", trial, "recalls", out["recalls"], "min gap", gap, "tol", tol, "max|s|", float(scores.abs().max()))


def run_configs():
    """the four task_finetune_irtr_* named configs of the reference's config file, read as data (assignments of literals)"""
    src = open(os.path.join(G.REF, "vilt", "config.py")).read()
    tree = ast.parse(src)
    names = ("task_finetune_irtr_coco", "task_finetune_irtr_coco_randaug", "task_finetune_irtr_f30k", "task_finetune_irtr_f30k_randaug")
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            vals = {}
            for st in node.body:
                if isinstance(st, ast.Assign) and len(st.targets) == 1 and isinstance(st.targets[0], ast.Name):
                    key = st.targets[0].id
                    if key == "loss_names":                               # _loss_names({...}): the dict literal inside the call
                        vals[key] = ast.literal_eval(st.value.args[0])
                    else:
                        vals[key] = ast.literal_eval(st.value)
            out[node.name] = vals
    assert set(out) == set(names)
    with open(os.path.join(GOLD, "irtr_configs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("irtr_configs.json", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or R.FIXTURES + ("two_step", "recall", "configs")):
        {"two_step": run_two_step, "recall": run_recall, "configs": run_configs}.get(name, lambda n=name: run_step(n))()
