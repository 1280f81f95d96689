"""CPU: the host-side layout of the MLM head - state-dict names and shapes against the reference's MLMHead (recorded by
tools/gen_golden_mlm.py), the arena specs of models without the head against a recorded list, the AdamW groups of the six tensors
(vilt_utils.py:335-393) and the two task configs against the reference's values (config.py:202-221, recorded data)."""
import ctypes as C
import json
import os

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd.runtime import make_dims, param_specs, mlm_layout
from rmcl_amd.vilt import config as CFG
from rmcl_amd.vilt.modules.vilt_utils import adamw_segments
from tests import mlm_oracle as M
from tests.golden_util import GOLDEN


def _layout(cfg):
    d = make_dims(cfg, 1, L.F32, True)
    lay = L.Layout()
    L.lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    return lay


def test_state_dict_names_and_shapes_equal_the_reference_head():
    ref = json.load(open(os.path.join(GOLDEN, "mlm_head_shapes.json")))
    cfg = CFG.task_mlm_itm()
    head, specs, used = mlm_layout(cfg, 0)
    assert {n: list(s) for n, _, s in specs} == ref
    assert dict(M.mlm_param_shapes(cfg)) == {n: tuple(s) for n, s in ref.items()}
    assert "mlm_score.decoder.bias" not in ref                       # Linear(D, V, bias=False) + a free bias [V]
    assert (head.D, head.V) == (768, 30522)


def test_head_slots_are_aligned_and_disjoint():
    cfg = CFG.task_mlm_itm()
    base = int(_layout(cfg).total) + 128
    head, specs, used = mlm_layout(cfg, base)
    end = base
    for name, off, shape in specs:
        n = 1
        for s in shape:
            n *= s
        assert off % 64 == 0 and off >= end, name
        end = off + n
    assert base + used >= end and used % 64 == 0
    assert [getattr(head, k) for k in ("tw", "tb", "lg", "lb", "dw", "db")] == [off for _, off, _ in specs]


def test_specs_of_models_without_the_head_equal_the_recorded_list():
    rec = json.load(open(os.path.join(GOLDEN, "mlm_specs_without_head.json")))
    for task, want in rec.items():
        cfg = getattr(CFG, task)(num_layers=2)
        lay = _layout(cfg)
        got = [[n, int(o), list(s)] for n, o, s in param_specs(cfg, lay)]
        assert got == want["specs"], task
        assert int(lay.total) == want["total"], task
        assert cfg["loss_names"]["mlm"] == 0


def test_adamw_groups_of_the_head():
    cfg = CFG.task_mlm_itm()
    head, specs, used = mlm_layout(cfg, 0)
    ends, mults, wds = adamw_segments(specs, used, 0.01, 10.0)
    got = {n: (m, w) for (n, _, _), m, w in zip(sorted(specs, key=lambda s: s[1]), mults, wds)}
    for n, (m, w) in got.items():
        assert m == 1.0, n                                            # mlm_score is not in head_names: base learning rate
        assert w == (0.01 if n.endswith(("dense.weight", "decoder.weight")) else 0.0), n      # bias / LayerNorm.* undecayed


def test_task_configs_hold_the_reference_values():
    ln = {"moco": 0, "barlowtwins": 0, "itm": 1, "mlm": 1, "mpp": 0, "vqa": 0, "nlvr2": 0, "irtr": 0, "irtr_attacked": 0,
          "nlvr2_attacked": 0, "vqa_attacked": 0}
    a = CFG.task_mlm_itm()
    assert (a["exp_name"], a["datasets"], a["loss_names"], a["batch_size"], a["max_epoch"], a["max_image_len"]) == \
        ("mlm_itm", ["coco"], ln, 4096, 10, 200)
    b = CFG.task_mlm_itm_randaug()
    assert (b["exp_name"], b["datasets"], b["train_transform_keys"], b["loss_names"], b["batch_size"], b["max_epoch"], b["max_image_len"]) == \
        ("mlm_itm_randaug", ["coco", "vg", "sbu", "gcc"], ["pixelbert_randaug"], ln, 4096, 10, 200)
    for cfg in (a, b):                                                 # everything else: the defaults (mlm_prob 0.15, no whole-word masking)
        assert cfg["mlm_prob"] == 0.15 and cfg["whole_word_masking"] is False and cfg["vocab_size"] == 30522 and cfg["max_text_len"] == 40
    assert CFG.task_mlm_itm(per_gpu_batchsize=4)["per_gpu_batchsize"] == 4
