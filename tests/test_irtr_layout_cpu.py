"""CPU: the host-side pieces of image-text retrieval - the rank split against torch's DistributedSampler, the recall function on the
fixture's score matrix, the arena layout (rank_output is a view of row 1 of the ITM head; every other model keeps its layout), the
AdamW segments, the tile schedule and the four task configs against the reference's values (recorded data)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DistributedSampler

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd.runtime import make_dims, param_specs, irtr_alias_specs, is_irtr
from rmcl_amd.vilt import config as CFG
from rmcl_amd.vilt.modules import objectives
from tests import irtr_oracle as R
from tests.golden_util import GOLDEN


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 2, 5, 7, 8, 16, 17, 24, 500])
def test_rank_split_equals_distributed_sampler(n, world):
    seen = []
    for rank in range(world):
        ref = list(DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=False))
        got = objectives.irtr_rank_split(n, world, rank)
        assert got == ref, (n, world, rank)
        seen += got
    assert len(seen) == -(-n // world) * world and set(seen) == set(range(n))       # padded by wrap-around, nothing dropped


def test_recall_function_returns_the_fixture_values_exactly():
    g = R.load(R.RECALL)
    scores = torch.from_numpy(g["scores"])
    iids, tiids = torch.from_numpy(g["iids"]), torch.from_numpy(g["tiids"])
    got = objectives.irtr_recall_from_scores(scores, iids, tiids)
    assert [float(x) for x in got] == [float(x) for x in g["recalls"]]
    assert [float(x) for x in R.recall_from_scores(scores, iids, tiids)] == [float(x) for x in g["recalls"]]
    # duplicate image rows (the sampler's wrap-around padding) are counted, as in the reference's gathered matrix
    dup = objectives.irtr_recall_from_scores(torch.cat([scores, scores[:2]]), torch.cat([iids, iids[:2]]), tiids)
    ref = R.recall_from_scores(torch.cat([scores, scores[:2]]), torch.cat([iids, iids[:2]]), tiids)
    assert [float(x) for x in dup] == [float(x) for x in ref]


def test_fixture_decision_boundaries_are_clear():
    g = R.load(R.RECALL)
    s = torch.from_numpy(g["scores"])
    tol = R.TOL_SCORE_F32 * max(1.0, float(s.abs().max()))
    assert s.shape[0] > 10 and s.shape[1] > 10                       # an 11th score in every row and column: the R@10 boundary exists
    gaps = []
    for dim in (0, 1):
        v = s.sort(dim=dim, descending=True).values
        for k in (1, 5, 10):
            gaps.append(float((v.narrow(dim, k - 1, 1) - v.narrow(dim, k, 1)).min()))
    assert len(gaps) == 6 and min(gaps) >= 20 * tol and abs(min(gaps) - float(g["min_gap"])) < 1e-6
    # R@10 is not trivial in either direction: below 1, below the share of images that have a caption, and different from R@5
    rec = [float(x) for x in g["recalls"]]
    with_caption = len(set(g["tiids"].tolist())) / s.shape[0]
    assert 0 < rec[2] < 1 and 0 < rec[5] < with_caption and rec[2] != rec[1] and rec[5] != rec[4] and len(set(rec)) == 6
    # and it depends on k and on the index arrays: the wrong k, or the caption indices read as image indices, give other values
    iids, tiids = torch.from_numpy(g["iids"]), torch.from_numpy(g["tiids"])
    own = iids.view(-1, 1) == tiids.view(1, -1)
    for k_wrong in (9, 11):
        assert float(own.gather(1, s.topk(k_wrong, dim=1).indices).any(dim=1).float().mean()) != rec[5] or \
            float(own.gather(0, s.topk(k_wrong, dim=0).indices).any(dim=0).float().mean()) != rec[2]


def _layout(cfg):
    d = make_dims(cfg, 2, 0, True)
    lay = L.Layout()
    L.lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    return lay


def test_models_without_irtr_keep_their_arena():
    for cfg in (CFG.task_moco(), CFG.task_finetune_vqa(), CFG.default_config()):
        lay = _layout(cfg)
        assert not is_irtr(cfg) and irtr_alias_specs(cfg, lay) == []
        specs = param_specs(cfg, lay)
        assert len(specs) == 165 and int(lay.total) == 112287040 and int(lay.itm_w) == 112285440 and int(lay.itm_b) == 112286976
        assert not any(n.startswith("rank_output") for n, _, _ in specs)


def test_rank_output_views_sit_on_row_1_of_the_itm_head():
    cfg = CFG.task_finetune_irtr_coco()
    lay = _layout(cfg)
    base = _layout(CFG.task_moco())
    assert {f: getattr(lay, f) for f in L.LAYOUT_FIELDS} == {f: getattr(base, f) for f in L.LAYOUT_FIELDS}      # no new arena space
    assert param_specs(cfg, lay) == param_specs(CFG.task_moco(), base)
    al = dict((n, (off, shape)) for n, off, shape in irtr_alias_specs(cfg, lay))
    D = cfg["hidden_size"]
    assert al["rank_output.weight"] == (int(lay.itm_w) + D, (1, D))
    assert al["rank_output.bias"] == (int(lay.itm_b) + 1, (1,))
    assert (int(lay.itm_w) + D) % 64 == 0                       # row 1 starts an AdamW segment of its own (64-element aligned)


def test_adamw_segments_freeze_row_0_and_decay_row_1():
    from rmcl_amd.vilt.modules.vilt_utils import adamw_segments
    wd, lr_mult = 0.01, 10.0
    for cfg in (CFG.task_moco(loss_names=CFG._loss_names({"moco": 1, "itm": 1})), CFG.task_finetune_vqa()):
        lay = _layout(cfg)
        specs = param_specs(cfg, lay)
        ends, mults, wds = adamw_segments(specs, int(lay.total), wd, lr_mult, is_irtr(cfg))
        assert len(ends) == len(specs) and ends[-1] == int(lay.total)                   # one segment per tensor, as before
        i = [n for n, _, _ in sorted(specs, key=lambda t: t[1])].index("itm_score.fc.weight")
        assert (mults[i], wds[i]) == (1.0, wd)
    cfg = CFG.task_finetune_irtr_coco()
    lay = _layout(cfg)
    specs = param_specs(cfg, lay)
    D = cfg["hidden_size"]
    ends, mults, wds = adamw_segments(specs, int(lay.total), wd, lr_mult, True)
    base = adamw_segments(specs, int(lay.total), wd, lr_mult, False)
    assert len(ends) == len(specs) + 1 and ends == sorted(ends) and all(e % 4 == 0 for e in ends)
    seg = {e: (m, w) for e, m, w in zip(ends, mults, wds)}
    assert seg[int(lay.itm_w) + D] == (0.0, 0.0)                     # row 0 of the ITM weight: no step, no decay
    assert seg[int(lay.itm_b)] == (1.0, wd)                          # row 1 = rank_output.weight: base learning rate (not a head), decayed
    assert seg[int(lay.total)] == (1.0, 0.0)                         # itm_score.fc.bias / rank_output.bias: stepped, not decayed
    others = [(e, m, w) for e, m, w in zip(ends, mults, wds) if e not in (int(lay.itm_w) + D, int(lay.itm_b))]
    assert others == [(e, m, w) for e, m, w in zip(*base) if e != int(lay.itm_b)]        # every other segment as without irtr


def test_tile_schedule_covers_every_pair_once_and_pads_to_the_tile():
    counts = [144, 120, 144, 88, 120, 132, 144]
    seen = {}
    for grp, n, t0, t1 in objectives.irtr_tiles(counts, 10, 3, 4):
        assert n == max(counts[i] for i in grp) and len(grp) <= 3 and 0 < t1 - t0 <= 4
        for i in grp:
            for t in range(t0, t1):
                seen[(i, t)] = seen.get((i, t), 0) + 1
    assert len(seen) == 7 * 10 and set(seen.values()) == {1}
    firsts = [grp for grp, _, t0, _ in objectives.irtr_tiles(counts, 10, 3, 4) if t0 == 0]
    assert firsts == [[3, 1, 4], [5, 0, 2], [6]]                # sorted by patch count, ties by index


def test_configs_equal_the_reference_values():
    ref = json.load(open(os.path.join(GOLDEN, "irtr_configs.json")))
    assert sorted(ref) == ["task_finetune_irtr_coco", "task_finetune_irtr_coco_randaug", "task_finetune_irtr_f30k", "task_finetune_irtr_f30k_randaug"]
    for name, vals in ref.items():
        cfg = getattr(CFG, name)()
        for k, v in vals.items():
            if k == "loss_names":
                assert cfg[k] == CFG._loss_names(v), (name, k)
            else:
                assert cfg[k] == v, (name, k, cfg[k], v)
        assert cfg["loss_names"]["irtr"] == 1 and cfg["loss_names"]["itm"] == 0.5 and cfg["draw_false_text"] == 15 and cfg["get_recall_metric"] is True
