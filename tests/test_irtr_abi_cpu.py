"""CPU: the argument checks of the image-text retrieval entry points (include/rmcl.h "Image-text retrieval") return an error code and a
message before anything is launched or dereferenced - NULL operands, shapes the kernels do not cover, a cache slot shorter than the pass."""
import ctypes as C

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L

lib = L.lib
F = C.c_float


def _err(rc, needle):
    assert rc != 0
    msg = lib.rmcl_last_error().decode()
    assert needle in msg, msg


def _dims(**kw):
    base = dict(B=4, L=40, P=144, D=768, H=12, layers=2, mlp=3072, patch_k=3072, proj=128, vocab=30522, dtype=L.F32, exact=1, Pp=144)
    base.update(kw)
    return L.Dims(**base)


def test_rank_head_entry_points_check_their_arguments():
    one = (C.c_float * 8)()
    _err(lib.rmcl_irtr_score(None, L.I64(768), one, one, 4, 768, one, None, L.I64(4), None), "irtr_score: NULL")
    _err(lib.rmcl_irtr_score(one, L.I64(768), one, one, 4, 770, one, None, L.I64(4), None), "irtr_score: bad shape")
    _err(lib.rmcl_irtr_score(one, L.I64(512), one, one, 4, 768, one, None, L.I64(4), None), "irtr_score: bad shape")
    _err(lib.rmcl_irtr_score(one, L.I64(768), one, one, 4, 768, one, None, L.I64(3), None), "fewer than S")
    _err(lib.rmcl_irtr_ce(None, 2, 4, F(1.0), None, None, None, one, None), "irtr_ce: NULL")
    _err(lib.rmcl_irtr_ce(one, 2, 65, F(1.0), None, None, None, one, None), "irtr_ce: bad shape")
    _err(lib.rmcl_irtr_ce(one, 0, 4, F(1.0), None, None, None, one, None), "irtr_ce: bad shape")
    _err(lib.rmcl_irtr_bwd(one, one, L.I64(768), one, 4, 768, None, None, None, None), "irtr_bwd: NULL")
    _err(lib.rmcl_irtr_bwd(one, one, L.I64(768), one, 4, 766, one, None, None, None), "irtr_bwd: bad shape")


def test_rank_pass_and_visual_embed_check_their_arguments():
    d = _dims()
    one = (C.c_float * 8)()
    p = C.cast(one, C.c_void_p)
    _err(lib.rmcl_visual_embed(C.byref(d), None, None, None, None, None, None, None, None), "visual_embed: NULL")
    _err(lib.rmcl_visual_embed(C.byref(_dims(P=100)), p, None, p, None, p, p, p, None), "needs the rmcl_ragged selection")
    _err(lib.rmcl_encoder_forward_rank(C.byref(d), L.MODE_INFER, p, None, p, p, None, p, p, p, None, None), "encoder_forward_rank: NULL")
    src = L.RankSrc(embeds=p.value, masks=p.value, img_of=p.value, n_img=1, ld_tok=145)
    _err(lib.rmcl_encoder_forward_rank(C.byref(d), L.MODE_FULL, p, None, p, p, C.byref(src), p, p, p, None, None), "INFER mode only")
    short = L.RankSrc(embeds=p.value, masks=p.value, img_of=p.value, n_img=1, ld_tok=144)
    _err(lib.rmcl_encoder_forward_rank(C.byref(d), L.MODE_INFER | L.MODE_CLS_TAIL, p, None, p, p, C.byref(short), p, p, p, None, None),
         "fewer than 1 + P token rows")
    _err(lib.rmcl_encoder_forward_rank(C.byref(_dims(n_types=3, img_type=2)), L.MODE_INFER, p, None, p, p, C.byref(src), p, p, p, None, None),
         "token-type row 1")
