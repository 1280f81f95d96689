"""CPU: the token-type fields of rmcl_dims (include/rmcl.h n_types / img_type).  A zero-initialised Dims gives exactly the pre-training
layout; n_types = 3 makes token_type_embeddings a contiguous [3, D] block and shifts every later tensor by the same D elements."""
import ctypes as C

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd.runtime import make_dims, param_specs, nlvr2_layout
from rmcl_amd.vilt.config import task_finetune_nlvr2, task_moco, task_finetune_vqa


def _layout(**kw):
    d = L.Dims(B=2, L=40, P=144, D=768, H=12, layers=12, mlp=3072, patch_k=3072, proj=128, vocab=30522, dtype=0, exact=1, Pp=144, **kw)
    lay = L.Layout()
    L.lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    return {f: getattr(lay, f) for f in L.LAYOUT_FIELDS}


def test_default_dims_keep_the_pretraining_layout():
    base = _layout()
    assert base == _layout(n_types=0, img_type=0) == _layout(n_types=2, img_type=1) == _layout(n_types=0, img_type=-1)
    assert base["ema_end"] == 111694848 and base["cls"] == base["vtype"] + 2 * 768
    for cfg in (task_moco(), task_finetune_vqa()):
        d = make_dims(cfg, 2, 0, True)
        assert d.n_types == 0 and d.img_type == 0


def test_three_token_types_shift_everything_after_by_d():
    base, three = _layout(), _layout(n_types=3)
    before = ("word", "pos", "btype", "eln_w", "eln_b", "vtype")
    relative = ("layer_stride", "ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
    for f in L.LAYOUT_FIELDS:
        if f in before or f in relative:
            assert three[f] == base[f], f
        else:
            assert three[f] == base[f] + 768, f
    assert three["cls"] == three["vtype"] + 3 * 768                  # the [3, D] table is contiguous


def test_nlvr2_specs_are_disjoint_and_ordered():
    cfg = task_finetune_nlvr2()
    d = make_dims(cfg, 2, 0, True)
    assert d.n_types == 3
    lay = L.Layout()
    L.lib.rmcl_param_layout(C.byref(d), C.byref(lay))
    specs = param_specs(cfg, lay)
    h, hs, n = nlvr2_layout(cfg, int(lay.total))
    specs = specs + hs
    tt = [s for s in specs if s[0] == "token_type_embeddings.weight"][0]
    assert tt[2] == (3, 768) and tt[1] == lay.vtype
    spans = sorted((off, off + (lambda s: __import__("math").prod(s))(shape), name) for name, off, shape in specs)
    for (a0, a1, na), (b0, b1, nb) in zip(spans, spans[1:]):
        assert a1 <= b0, (na, nb)
    assert h.D == h.H == 1536 and h.N == 2 and h.ldl == 64
    assert dict((s[0], s[2]) for s in hs)["nlvr2_classifier.3.weight"] == (2, 1536)
    assert hs[0][1] == lay.total and n >= 1536 * 1536 + 64 * 1536
