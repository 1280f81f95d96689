"""CPU: RandAugment, host side.  The numpy restatement (vilt/transforms/randaug_model.py - the specification csrc/randaug.hip is written
from) against PIL byte for byte; the plan draws and the PIL execution against the reference's recorded runs (tests/golden/randaug.npz,
written by tools/gen_golden_randaug.py from the reference's own randaug.py); the two new transform keys, the batch plumbing, the argument
checks of rmcl_randaug_u8 / rmcl_randaug_scratch_bytes (host buffers: the checks precede any launch) and the kernels' scratch use."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib
from rmcl_amd.attack import word_substitution as WS
from rmcl_amd.vilt import config as CFG
from rmcl_amd.vilt.datasets import BaseDataset, RawUint8Batch
from rmcl_amd.vilt.datasets.base_dataset import RawView, collate_raw_uint8
from rmcl_amd.vilt.transforms import keys_to_transforms
from rmcl_amd.vilt.transforms import randaug as R
from rmcl_amd.vilt.transforms import randaug_model as M
from tests import randaug_util as U
from tests.golden_util import digest, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def pil_bytes(img, code, v):
    return np.asarray(R.apply_op_pil(Image.fromarray(img), code, v))


def model_bytes(img, code, v):
    ops, params = R.plan_params([(code, v)], img.shape[1], img.shape[0])
    return M.apply_op(img, ops[0], params[0])


# ---------------------------------------------------------------------------------------------------------------------
# the model against PIL
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", U.SIZES)
def test_model_equals_pil_for_every_op(w, h):
    """all 14 ops at m = 9, 21, 30 (m = 21 is the factor at which a fused multiply-add would change blend bytes), both signs, on noise over
    the whole byte range and on a smooth-plus-noise image whose histograms end inside it"""
    for make in (U.noise_image, U.smooth_image):
        img = make(w, h, 1000 * w + h)
        for code, m, v in U.single_cases():
            want, got = pil_bytes(img, code, v), model_bytes(img, code, v)
            assert np.array_equal(want, got), (R.OPS[code][1], m, v, make.__name__, int((want != got).sum()))


def test_model_equals_pil_on_degenerate_histograms():
    """a constant channel (identity tables), a two-valued channel (AutoContrast stretches it to 0 / 255, Equalize's step is the count of the
    lower value // 255) and a channel whose Equalize step is 0 (fewer than 255 pixels below the last bin)"""
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (40, 52, 3), dtype=np.uint8)
    img[..., 0] = 77                                                       # constant
    img[..., 1] = np.where(rng.random((40, 52)) < 0.4, 30, 200)            # two values
    few = np.full((40, 52), 250, np.uint8)                                 # step 0: 100 pixels below the last non-empty bin
    few.ravel()[:100] = rng.integers(0, 250, 100)
    img[..., 2] = few
    hist = M.histograms(img)
    assert (hist[2].sum() - hist[2][250]) // 255 == 0 and np.count_nonzero(hist[0]) == 1 and np.count_nonzero(hist[1]) == 2
    for code in (R.AUTOCONTRAST, R.EQUALIZE, R.CONTRAST):
        for m in U.MAGNITUDES:
            v = R.magnitude(code, m)
            assert np.array_equal(pil_bytes(img, code, v), model_bytes(img, code, v)), (code, m)
    tiny = rng.integers(0, 256, (2, 2, 3), dtype=np.uint8)                 # 4 pixels: every Equalize step is 0
    assert np.array_equal(pil_bytes(tiny, R.EQUALIZE, 0.3), model_bytes(tiny, R.EQUALIZE, 0.3))


def test_autocontrast_table_for_every_lo_hi_pair():
    """all 32 640 (lo, hi) pairs with lo < hi against the Python expression of ImageOps.autocontrast"""
    n = 0
    for lo in range(256):
        for hi in range(lo + 1, 256):
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            want = [min(max(int(ix * scale + offset), 0), 255) for ix in range(256)]
            assert M.autocontrast_table(lo, hi).tolist() == want, (lo, hi)
            n += 1
    assert n == 32640
    # and PIL itself on a few two-valued single-channel images
    for lo, hi in ((0, 255), (3, 250), (17, 18), (100, 227), (254, 255)):
        band = np.array([[lo, hi], [hi, lo]], np.uint8)
        got = np.asarray(ImageOps.autocontrast(Image.fromarray(band)))
        assert np.array_equal(got, M.autocontrast_table(lo, hi)[band])


def test_blend_is_unfused_float32():
    """the model's blend for every (degenerate, source) byte pair against a blend computed in float64 and rounded ONCE (what a fused
    multiply-add returns): at factor 1.36 they must differ somewhere - the case that tells a fused kernel from PIL's arithmetic"""
    d, s = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    f = np.float32(R.magnitude(R.COLOR, 21))
    fused = (d.astype(np.float64) + np.float64(f) * (s.astype(np.float64) - d.astype(np.float64))).astype(np.float32)
    assert int((M.blend(d, s, float(f)) != M.clip8(fused)).sum()) > 0
    got = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(s), float(f)))
    assert np.array_equal(got, M.blend(d, s, float(f)))


# ---------------------------------------------------------------------------------------------------------------------
# the plan against the reference's recorded runs
# ---------------------------------------------------------------------------------------------------------------------

def test_op_table_is_the_references_list():
    g = load("randaug.npz")
    assert [n for _, n, _, _, _ in R.OPS] == g["op_names"].tolist()
    assert [float(lo) for _, _, lo, _, _ in R.OPS] == g["op_min"].tolist() and [float(hi) for _, _, _, hi, _ in R.OPS] == g["op_max"].tolist()
    assert [c for c, *_ in R.OPS] == list(range(14))


def test_seeded_draws_equal_the_references():
    """RandAugment(2, 9) under 40 seeds on both source images: op codes, signed values, the next random.random() after the call (the plan
    consumes the stream exactly as the reference does), the digest and the byte sample of PIL's output"""
    g = load("randaug.npz")
    images = U.fixture_images()
    assert int(g["sample_stride"]) == U.SAMPLE_STRIDE and g["img_sizes"].tolist() == [list(s) for s in U.FIXTURE_SIZES]
    for k, im in enumerate(images):
        np.testing.assert_array_equal(digest(torch.from_numpy(im)), g["img_digest"][k])
        for j, seed in enumerate(g["draw_seeds"].tolist()):
            random.seed(seed)
            plan = R.draw_plan(2, 9)
            assert random.random() == g["draw_next_random"][k, j], (k, seed)
            assert [c for c, _ in plan] == g["draw_codes"][k, j].tolist() and [v for _, v in plan] == g["draw_values"][k, j].tolist(), (k, seed)
            out = np.asarray(R.apply_plan_pil(Image.fromarray(im), plan))
            assert np.array_equal(U.strided(out), g[f"draw_sample_{k}"][j]), (k, seed, plan)
            np.testing.assert_array_equal(digest(torch.from_numpy(out.copy())), g[f"draw_digest_{k}"][j])
            assert np.array_equal(M.apply_plan(im, plan), out), (k, seed, plan)         # and the model, stage after stage
            random.seed(seed)                                                            # the transform object itself: same stream, same bytes
            assert np.array_equal(np.asarray(R.RandAugment(2, 9)(Image.fromarray(im))), out)


def test_single_op_records_equal_the_references():
    g = load("randaug.npz")
    cases = U.single_cases()
    assert [c for c, _, _ in cases] == g["single_codes"].tolist() and [m for _, m, _ in cases] == g["single_m"].tolist()
    assert [v for _, _, v in cases] == g["single_values"].tolist()
    for k, im in enumerate(U.fixture_images()):
        for j, (code, m, v) in enumerate(cases):
            out = pil_bytes(im, code, v)
            assert np.array_equal(U.strided(out), g[f"single_sample_{k}"][j]), (k, R.OPS[code][1], m, v)
            np.testing.assert_array_equal(digest(torch.from_numpy(out.copy())), g[f"single_digest_{k}"][j])
            ops, params = R.plan_params([(code, v)], im.shape[1], im.shape[0])
            assert np.array_equal(np.asarray(R.apply_params_pil(Image.fromarray(im), ops, params)), out)   # the device encoding, run by PIL


def test_plan_params_rejects_what_the_device_does_not_cover():
    for bad in ([(R.ROTATE, 90.0)], [(R.ROTATE, -180.0)], [(14, 1.0)], [], [(R.COLOR, 1.0)] * 9, [(R.SHEAR_X, 0.0)]):
        with pytest.raises(ValueError):
            R.plan_params(bad, 64, 48)
    with pytest.raises(ValueError):
        R.plan_params([(R.ROTATE, 9.0)], 20000, 48)
    ops, params = R.plan_params([(R.POSTERIZE, 1.2), (R.TRANSLATE_Y, -30.0)], 64, 48)
    assert ops.tolist() == [3, 13] and params[0, 0] == 1.0 and params[1].tolist() == [1, 0, 0, 0, 1, -30.0]


# ---------------------------------------------------------------------------------------------------------------------
# transform keys and batch plumbing
# ---------------------------------------------------------------------------------------------------------------------

RANDAUG_CONFIGS = ("task_finetune_vqa_randaug", "task_finetune_vqa_randaug_attacked", "task_finetune_nlvr2_randaug",
                   "task_finetune_nlvr2_randaug_attacked", "task_finetune_irtr_coco_randaug", "task_finetune_irtr_f30k_randaug", "task_mlm_itm_randaug")


@pytest.mark.parametrize("name", RANDAUG_CONFIGS)
def test_the_randaug_configs_build_their_train_transform(name):
    cfg = getattr(CFG, name)()
    assert cfg["train_transform_keys"] == ["pixelbert_randaug"]
    (tr,) = keys_to_transforms(cfg["train_transform_keys"], size=cfg["image_size"])
    img = Image.fromarray(U.source_image(97, 131, 3))
    random.seed(11)
    got = tr(img)
    random.seed(11)
    want = keys_to_transforms(["pixelbert"], size=cfg["image_size"])[0](R.apply_plan_pil(img, R.draw_plan(2, 9)))
    assert got.dtype == torch.float32 and got.shape[0] == 3 and got.shape[1] % 32 == 0 and got.shape[2] % 32 == 0
    assert torch.equal(got, want)


def _dataset(transform, **kw):
    tok = WS.load_tokenizer(os.path.join(GOLD, "toy_vocab.txt"))
    return BaseDataset(GOLD, [transform], 96, ["toy_shard"], text_column_name="caption", tokenizer=tok, **kw)


def test_raw_collate_carries_the_plans_and_the_host_path_is_the_references_batch():
    """"decode_uint8_randaug" + collate_raw_uint8 -> RawUint8Batch.aug; augmented and resized on the host it is, bit for bit, the float batch of
    "pixelbert_randaug" under the same seed (both keys consume `random` alike)"""
    raw_ds = _dataset("decode_uint8_randaug", remove_duplicate=False, draw_false_image=1)
    ref_ds = _dataset("pixelbert_randaug", remove_duplicate=False, draw_false_image=1)
    idx = [0, 2, 5, 8]
    random.seed(5)
    rb = raw_ds.collate([raw_ds[i] for i in idx])
    after_raw = random.random()
    random.seed(5)
    fb = ref_ds.collate([ref_ds[i] for i in idx])
    assert random.random() == after_raw
    changed = 0
    for key in ("image", "false_image_0"):
        r, f = rb[key][0], fb[key][0]
        assert isinstance(r, RawUint8Batch) and r.aug is not None
        ops, params = r.aug
        assert ops.dtype == torch.int32 and tuple(ops.shape) == (len(idx), 2) and params.dtype == torch.float64 and tuple(params.shape) == (len(idx), 2, 6)
        assert int(ops.min()) >= 0 and int(ops.max()) <= 13
        moved = r.to("cpu")
        assert moved.aug is not None and torch.equal(moved.aug[0], ops) and torch.equal(moved.aug[1], params)
        assert tuple(r.shape) == tuple(f.shape) and torch.equal(r.float_image(), f)
        plain = RawUint8Batch(r.data, r.sizes, r.shorter, r.longer, r.extent)
        changed += int(not torch.equal(plain.resized_on_host().data, r.resized_on_host().data))
    assert changed > 0                                                       # (the plans do something)
    # without a plan nothing changes: the plain key gives aug None
    plain_ds = _dataset("decode_uint8", remove_duplicate=False)
    assert plain_ds.collate([plain_ds[i] for i in idx])["image"][0].aug is None


def test_raw_collate_wants_all_or_no_plans_and_one_length():
    px = torch.zeros(8, 8, 3, dtype=torch.uint8)
    mk = lambda plan: {"image": [RawView(px, 96, 159, plan=plan)]}
    one, two = [(R.COLOR, 1.36)], [(R.COLOR, 1.36), (R.SOLARIZE, 76.8)]
    assert collate_raw_uint8([mk(two), mk(two)])["image"][0].aug[0].tolist() == [[6, 4], [6, 4]]
    for bad in ([mk(two), mk(None)], [mk(one), mk(two)]):
        with pytest.raises(AssertionError):
            collate_raw_uint8(bad)
    with pytest.raises(ValueError):
        RawUint8Batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.tensor([[8, 8], [8, 8]]), 96, 159, aug=(torch.tensor([[14], [0]]), torch.zeros(2, 1, 6)))
    with pytest.raises(ValueError):
        RawUint8Batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.tensor([[8, 8], [8, 8]]), 96, 159, aug=(torch.zeros(1, 1), torch.zeros(1, 1, 6)))


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points without a GPU
# ---------------------------------------------------------------------------------------------------------------------

def _rejected(rc, *words):
    assert rc == -1
    msg = _lib.lib.rmcl_last_error()
    assert msg and b"randaug" in msg and all(w.encode() in msg for w in words), msg


def test_randaug_arguments_are_rejected_before_any_launch():
    """rmcl_randaug_u8: every operand as NULL, dst / tmp aliasing src (or each other), an op code outside 0..13, n_ops outside 1..8.  Host
    buffers throughout: a wrapper that got past its check would launch on them."""
    lib = _lib.lib
    B, Hs, Ws, n = 2, 4, 4, 2
    src, tmp, dst = ((C.c_uint8 * (B * Hs * Ws * 3))() for _ in range(3))
    scratch = (C.c_uint8 * 16384)()
    sizes = (C.c_int32 * (2 * B))(4, 4, 4, 4)
    ops = (C.c_int32 * (B * n))(0, 13, 6, 9)
    params = (C.c_double * (B * n * 6))()
    good = [src, sizes, B, Hs, Ws, ops, params, n, tmp, scratch, dst, None]
    for i in (0, 1, 5, 6, 8, 9, 10):
        a = list(good)
        a[i] = None
        _rejected(lib.rmcl_randaug_u8(*a), "NULL")
    for i, j in ((10, 0), (8, 0), (10, 8)):                                   # dst = src, tmp = src, dst = tmp
        a = list(good)
        a[i] = a[j]
        _rejected(lib.rmcl_randaug_u8(*a), "alias")
    a = list(good)
    a[10] = C.cast(C.addressof(src) + 3, C.c_void_p)                           # dst overlapping src
    _rejected(lib.rmcl_randaug_u8(*a), "alias")
    for code in (-1, 14, 1 << 20):
        a = list(good)
        a[5] = (C.c_int32 * (B * n))(0, 13, code, 9)
        _rejected(lib.rmcl_randaug_u8(*a), "op code")
    for bad_n in (0, 9, -2):
        a = list(good)
        a[7] = bad_n
        _rejected(lib.rmcl_randaug_u8(*a), "n_ops")
    # the scratch query: grows with B and n_ops, 0 for what the call would reject
    s11, s12, s21 = (lib.rmcl_randaug_scratch_bytes(b, k) for b, k in ((1, 1), (1, 2), (2, 1)))
    assert 0 < s11 < s12 and s11 < s21 and s11 >= 3 * 256 * 4 + 8 + 768
    assert lib.rmcl_randaug_scratch_bytes(4, 0) == 0 and lib.rmcl_randaug_scratch_bytes(4, 9) == 0 and lib.rmcl_randaug_scratch_bytes(0, 2) == 0


def test_header_op_codes_are_the_plans():
    text = open(os.path.join(ROOT, "include", "rmcl.h")).read()
    codes = dict(re.findall(r"#define RMCL_RA_([A-Z_]+) (\d+)", text))
    want = {"AUTOCONTRAST": R.AUTOCONTRAST, "EQUALIZE": R.EQUALIZE, "ROTATE": R.ROTATE, "POSTERIZE": R.POSTERIZE, "SOLARIZE": R.SOLARIZE,
            "SOLARIZE_ADD": R.SOLARIZE_ADD, "COLOR": R.COLOR, "CONTRAST": R.CONTRAST, "BRIGHTNESS": R.BRIGHTNESS, "SHARPNESS": R.SHARPNESS,
            "SHEAR_X": R.SHEAR_X, "SHEAR_Y": R.SHEAR_Y, "TRANSLATE_X": R.TRANSLATE_X, "TRANSLATE_Y": R.TRANSLATE_Y, "MAX_OPS": R.MAX_OPS}
    assert {k: int(v) for k, v in codes.items()} == want


# ---------------------------------------------------------------------------------------------------------------------
# the kernels use no scratch memory (the reading of the compiler's assembly of tests/test_mpp_isa_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------

CSRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]


def test_randaug_kernels_use_no_scratch():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "randaug.s")
        r = subprocess.run(["hipcc", *FLAGS, os.path.join(CSRC, "randaug.hip"), "-o", dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        isa = open(dst).read()
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    names = " ".join(n for n, _ in sizes)
    for k in ("randaug_stats_kernel", "randaug_table_kernel", "randaug_apply_kernel"):
        assert k in names, (k, names[:400])
    spilled = [(n[:80], int(s)) for n, s in sizes if int(s) != 0]
    assert not spilled, spilled
