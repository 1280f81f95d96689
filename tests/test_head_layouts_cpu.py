"""CPU: the arena layouts of the four optional heads (Barlow-Twins, VQA, NLVR2, MLM) against a recorded list: struct fields, specs and
elements used of every ``*_layout(cfg, base)``, for the default config at base 0 and behind the encoder's tensors, and for a 2-layer
config whose widths are not multiples of 64 (the slot rounding shows).  tests/golden/head_layouts.json holds the recorded values."""
import ctypes as C
import json
import os

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd.runtime import make_dims, bt_layout, vqa_layout, nlvr2_layout, mlm_layout
from rmcl_amd.vilt.config import default_config
from tests.golden_util import GOLDEN

LAYOUTS = {"bt": bt_layout, "vqa": vqa_layout, "nlvr2": nlvr2_layout, "mlm": mlm_layout}


def _total(cfg) -> int:
    d = make_dims(cfg, 1, L.F32, True)
    lay = L.Layout()
    L.lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    return int(lay.total)


def _cases():
    full = default_config()
    small = default_config(num_layers=2, vqav2_label_size=100, vocab_size=1000, barlowtwins_dims=(256, 192, 100))
    return [("default@0", full, 0), ("default@total", full, _total(full)), ("small@total", small, _total(small))]


def snapshot():
    out = {}
    for case, cfg, base in _cases():
        for head, fn in LAYOUTS.items():
            st, specs, used = fn(cfg, base)
            out[f"{case}/{head}"] = {"base": base, "struct": {f: int(getattr(st, f)) for f, _ in st._fields_},
                                     "specs": [[n, int(o), list(s)] for n, o, s in specs], "used": int(used)}
    return out


def test_head_layouts_equal_the_recorded_list():
    want = json.load(open(os.path.join(GOLDEN, "head_layouts.json")))
    got = snapshot()
    assert sorted(got) == sorted(want) and len(got) == 12
    for key in want:
        assert got[key] == want[key], key
