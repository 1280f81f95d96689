"""CPU: the host-side layout of masked patch prediction - mpp_layout appends transformer.mask_token and the mpp_score tensors behind
every existing spec, a config without mpp yields exactly the recorded specs (tests/golden/head_layouts.json, mlm_specs_without_head.json),
the AdamW groups (vilt_utils.py:395-437), the task config against the reference's values (config.py:223-230) and the host mask draw."""
import ctypes as C
import json
import os

import torch

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd.runtime import make_dims, param_specs, mlm_layout, mpp_layout, mpp_draw_masks
from rmcl_amd.vilt import config as CFG
from rmcl_amd.vilt.modules.vilt_utils import adamw_segments
from tests import mpp_oracle as M
from tests.golden_util import GOLDEN


def _layout(cfg):
    d = make_dims(cfg, 1, L.F32, True)
    lay = L.Layout()
    L.lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    return lay


def test_mpp_layout_appends_behind_the_existing_specs():
    cfg = CFG.task_mlm_itm_mpp()
    lay = _layout(cfg)
    mh, mspecs, mused = mlm_layout(cfg, int(lay.total))
    base = int(lay.total) + mused
    head, specs, used = mpp_layout(cfg, base)
    assert [n for n, _, _ in specs] == M.HEAD and {n: tuple(s) for n, _, s in specs} == dict(M.mpp_param_shapes(cfg))
    end = base
    for name, off, shape in specs:
        n = 1
        for s in shape:
            n *= s
        assert off % 64 == 0 and off >= end, name
        end = off + n
    assert base + used >= end and used % 64 == 0 and head.D == 768
    assert [getattr(head, k) for k in ("mt", "tw", "tb", "lg", "lb", "dw", "db")] == [off for _, off, _ in specs]
    # the MLM head of the same model sits where it sits in a model without mpp (recorded layout)
    rec = json.load(open(os.path.join(GOLDEN, "head_layouts.json")))["default@total/mlm"]
    assert rec["base"] == int(lay.total) and [[n, int(o), list(s)] for n, o, s in mspecs] == rec["specs"] and mused == rec["used"]


def test_specs_of_models_without_mpp_equal_the_recorded_list():
    rec = json.load(open(os.path.join(GOLDEN, "mlm_specs_without_head.json")))
    for task, want in rec.items():
        cfg = getattr(CFG, task)(num_layers=2)
        lay = _layout(cfg)
        assert [[n, int(o), list(s)] for n, o, s in param_specs(cfg, lay)] == want["specs"], task
        assert int(lay.total) == want["total"] and cfg["loss_names"]["mpp"] == 0, task
    assert not any("mask_token" in n or "mpp_score" in n for n, _, _ in param_specs(CFG.task_mlm_itm(), _layout(CFG.task_mlm_itm())))


def test_adamw_groups_follow_the_reference_name_lists():
    cfg = CFG.task_mlm_itm_mpp()
    head, specs, used = mpp_layout(cfg, 0)
    ends, mults, wds = adamw_segments(specs, used, 0.01, 10.0)
    got = {n: (m, w) for (n, _, _), m, w in zip(sorted(specs, key=lambda s: s[1]), mults, wds)}
    for n, (m, w) in got.items():
        assert m == 1.0, n                                             # neither mask_token nor mpp_score is in head_names
        decayed = n in ("transformer.mask_token", "mpp_score.transform.dense.weight", "mpp_score.decoder.weight")
        assert w == (0.01 if decayed else 0.0), n                      # LayerNorm.* and *.bias are not decayed, mask_token is


def test_task_config_holds_the_reference_values():
    ln = {"moco": 0, "barlowtwins": 0, "itm": 1, "mlm": 1, "mpp": 1, "vqa": 0, "nlvr2": 0, "irtr": 0, "irtr_attacked": 0,
          "nlvr2_attacked": 0, "vqa_attacked": 0}
    a = CFG.task_mlm_itm_mpp()
    assert (a["exp_name"], a["datasets"], a["loss_names"], a["batch_size"], a["max_epoch"], a["max_image_len"]) == \
        ("mlm_itm_mpp", ["coco", "vg", "sbu", "gcc"], ln, 4096, 10, 200)
    assert a["mlm_prob"] == 0.15 and a["patch_size"] == 32 and a["image_size"] == 384 and a["drop_rate"] == 0.1
    assert CFG.task_mlm_itm_mpp(num_layers=2)["num_layers"] == 2


def test_mask_draw_equals_the_two_bernoulli_draws_in_the_reference_order():
    for s, (B, G) in ((0, (4, 144)), (7, (3, 12)), (123, (1, 1))):
        torch.manual_seed(s)
        masked, replaced = mpp_draw_masks(B, G)
        torch.manual_seed(s)
        a = torch.bernoulli(torch.full((B, G), 0.15)).bool()
        b = torch.bernoulli(torch.full((B, G), 0.8)).bool()
        assert torch.equal(masked, a) and torch.equal(replaced, b & a)
        assert masked.dtype == torch.bool and tuple(masked.shape) == (B, G)
