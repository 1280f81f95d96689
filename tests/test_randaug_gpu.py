"""-m gpu: RandAugment on the device (rmcl_randaug_u8, csrc/randaug.hip) against PIL itself - byte for byte inside every sample, zero outside -,
per op, composed, through Engine.resize_raw, and one training step on a device-augmented batch against the host-augmented one."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd._lib import lib, check, P  # noqa: E402
from rmcl_amd.vilt.datasets import RawUint8Batch  # noqa: E402
from rmcl_amd.vilt.transforms import randaug as R  # noqa: E402
from rmcl_amd.vilt.transforms import randaug_model as M  # noqa: E402
from tests import randaug_util as U  # noqa: E402

DEV = "cuda:0"
FILL = 0xA5                       # dst and tmp start as this byte: the zeros outside a sample must be written by the call


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack(images, Hs=None, Ws=None):
    """[h, w, 3] arrays -> (data uint8 [B, Hs, Ws, 3], sizes int32 [B, 2]), every sample in its top-left corner"""
    Hs, Ws = Hs or max(im.shape[0] for im in images), Ws or max(im.shape[1] for im in images)
    data = torch.zeros(len(images), Hs, Ws, 3, dtype=torch.uint8)
    for b, im in enumerate(images):
        data[b, : im.shape[0], : im.shape[1]] = torch.from_numpy(im)
    return data, torch.tensor([im.shape[:2] for im in images], dtype=torch.int32)


def device_randaug(data, sizes, ops, params):
    """rmcl_randaug_u8 on a packed batch; ops [B, n] / params [B, n, 6] numpy (the HOST arrays the entry point takes) -> dst on the host"""
    ops, params = np.ascontiguousarray(ops, np.int32), np.ascontiguousarray(params, np.float64)
    B, Hs, Ws, _ = data.shape
    n = ops.shape[1]
    assert ops.shape == (B, n) and params.shape == (B, n, 6)
    src, sz = data.to(DEV), sizes.to(DEV)
    tmp, dst = torch.full_like(src, FILL), torch.full_like(src, FILL)
    scratch = torch.empty(int(lib.rmcl_randaug_scratch_bytes(B, n)), dtype=torch.uint8, device=DEV)
    check(lib.rmcl_randaug_u8(P(src), P(sz), B, Hs, Ws, ops.ctypes.data_as(C.c_void_p), params.ctypes.data_as(C.c_void_p), n, P(tmp), P(scratch),
                              P(dst), stream()), "randaug_u8")
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), data)                                        # the source is read only
    return dst.cpu()


def plans_to_arrays(plans, images):
    packed = [R.plan_params(pl, im.shape[1], im.shape[0]) for pl, im in zip(plans, images)]
    return np.stack([o for o, _ in packed]), np.stack([p for _, p in packed])


def expect(images, plans, Hs, Ws):
    """PIL on every sample's own bytes, zero outside"""
    want = torch.zeros(len(images), Hs, Ws, 3, dtype=torch.uint8)
    for b, (im, pl) in enumerate(zip(images, plans)):
        want[b, : im.shape[0], : im.shape[1]] = torch.from_numpy(np.asarray(R.apply_plan_pil(Image.fromarray(im), pl)).copy())
    return want


def assert_same(got, want, images, what):
    for b, im in enumerate(images):
        h, w = im.shape[:2]
        g, x = got[b, :h, :w], want[b, :h, :w]
        assert torch.equal(g, x), (what, b, (w, h), int((g != x).sum()))
    assert torch.equal(got, want), (what, "bytes outside a sample must be zero")


@functools.lru_cache(maxsize=None)
def op_batch():
    """the nine edge sizes plus one 480 x 640 sample (Hs = 480, Ws = 640: padding, and several workgroups per sample), noise over the whole
    byte range and smooth-plus-noise images in turn"""
    images = [(U.noise_image if i % 2 == 0 else U.smooth_image)(w, h, 77 + i) for i, (w, h) in enumerate(U.SIZES)]
    images.append(U.smooth_image(640, 480, 5))
    images.append(U.noise_image(97, 131, 6))
    data, sizes = pack(images, 480, 640)
    return images, data, sizes


@pytest.mark.parametrize("code", range(14), ids=[n for _, n, *_ in R.OPS])
def test_every_op_gives_pils_bytes(code):
    """n_ops = 1, one op for the whole batch, at m = 9, 21, 30 (21: the blend factor at which a fused multiply-add changes bytes) and both signs"""
    images, data, sizes = op_batch()
    for c, m, v in U.single_cases():
        if c != code:
            continue
        plans = [[(code, v)]] * len(images)
        ops, params = plans_to_arrays(plans, images)
        got = device_randaug(data, sizes, ops, params)
        assert_same(got, expect(images, plans, 480, 640), images, (R.OPS[code][1], m, v))


def test_autocontrast_tables_on_the_device():
    """64 samples of 8 x 8 whose three channels each span a chosen (lo, hi): 192 table builds in one launch - the ends of the byte range,
    neighbouring values, a constant channel (identity) and a spread of pairs whose scale 255 / (hi - lo) is not exact"""
    rng = np.random.default_rng(12)
    pairs = [(0, 255), (0, 1), (254, 255), (0, 254), (1, 255), (127, 128), (5, 5), (3, 250), (17, 200), (100, 227), (64, 191), (0, 3)]
    while len(pairs) < 192:
        lo = int(rng.integers(0, 255))
        pairs.append((lo, int(rng.integers(lo, 256))))
    images = []
    for b in range(64):
        im = np.zeros((8, 8, 3), np.uint8)
        for c in range(3):
            lo, hi = pairs[3 * b + c]
            im[..., c] = rng.permutation(np.linspace(lo, hi, 64).round().astype(np.uint8)).reshape(8, 8)
        images.append(im)
    data, sizes = pack(images)
    for code in (R.AUTOCONTRAST, R.EQUALIZE):
        plans = [[(code, 0.3)]] * 64
        ops, params = plans_to_arrays(plans, images)
        assert_same(device_randaug(data, sizes, ops, params), expect(images, plans, 8, 8), images, R.OPS[code][1])


def small_images(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = int(rng.integers(20, 70)), int(rng.integers(20, 70))
        out.append((U.noise_image if i % 3 == 0 else U.smooth_image)(w, h, seed * 100 + i))
    return out


def signed_value(code, m, rng):
    v = R.magnitude(code, m)
    return -v if R.OPS[code][4] and rng.random() > 0.5 else v


@pytest.mark.parametrize("part", range(4))
def test_two_stage_plans_cover_every_ordered_pair(part):
    """n_ops = 2, a different plan per sample: all 14 x 14 ordered pairs over four batches of 49 samples"""
    rng = random.Random(part)
    pairs = [(a, b) for a in range(14) for b in range(14)][part * 49:(part + 1) * 49]
    images = small_images(len(pairs), 30 + part)
    plans = [[(a, signed_value(a, U.MAGNITUDES[i % 3], rng)), (b, signed_value(b, U.MAGNITUDES[(i // 3) % 3], rng))] for i, (a, b) in enumerate(pairs)]
    data, sizes = pack(images)
    ops, params = plans_to_arrays(plans, images)
    got = device_randaug(data, sizes, ops, params)
    assert_same(got, expect(images, plans, *data.shape[1:3]), images, ("pairs", part))
    if part == 0:                                                               # determinism: a second call, identical bytes
        assert torch.equal(device_randaug(data, sizes, ops, params), got)


def test_three_stage_plans_land_in_dst():
    """n_ops = 3: an odd stage count for the ping-pong src -> dst -> tmp -> dst; every op occurs at every stage"""
    rng = random.Random(9)
    images = small_images(28, 44)
    plans = [[((i + 5 * s) % 14, signed_value((i + 5 * s) % 14, U.MAGNITUDES[(i + s) % 3], rng)) for s in range(3)] for i in range(28)]
    for s in range(3):
        assert {pl[s][0] for pl in plans} == set(range(14))
    data, sizes = pack(images)
    ops, params = plans_to_arrays(plans, images)
    assert_same(device_randaug(data, sizes, ops, params), expect(images, plans, *data.shape[1:3]), images, "triples")
    for im, pl in zip(images[:6], plans[:6]):                                   # (and the numpy model agrees with both)
        assert np.array_equal(M.apply_plan(im, pl), np.asarray(R.apply_plan_pil(Image.fromarray(im), pl)))


# ---------------------------------------------------------------------------------------------------------------------
# through the engine
# ---------------------------------------------------------------------------------------------------------------------

def raw_batch_with_plans(sizes, seed, shorter=384, longer=640):
    images = [U.smooth_image(w, h, seed + i) for i, (h, w) in enumerate(sizes)]
    data, sz = pack(images)
    random.seed(seed)
    plans = [R.draw_plan(2, 9) for _ in images]
    ops, params = plans_to_arrays(plans, images)
    return RawUint8Batch(data, sz, shorter, longer, aug=(torch.from_numpy(ops), torch.from_numpy(params)))


def test_resize_raw_applies_the_plan_before_the_resize():
    from tests.test_parity2_gpu import make_module
    sizes = [(480, 640), (640, 480), (427, 640), (375, 500), (300, 451)]
    ocfg = O.default_config(num_layers=1, num_negative=256, per_gpu_batchsize=len(sizes), adv_steps_img=1)
    m, _ = make_module(ocfg, 5, "bf16")
    changed = 0
    for seed in (3, 4):
        raw = raw_batch_with_plans(sizes, seed)
        want = raw.resized_on_host()                                            # PIL: the plan, then the bicubic resize
        got = m.engine.resize_raw(raw.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(got.sizes, want.sizes) and torch.equal(got.data.cpu(), want.data)
        plain = RawUint8Batch(raw.data, raw.sizes, raw.shorter, raw.longer)
        changed += int(not torch.equal(plain.resized_on_host().data, want.data))
    assert changed == 2


def test_training_step_on_a_device_augmented_batch_equals_the_host_augmented_batch():
    """batch["image"] = RawUint8Batch with aug (what collate_raw_uint8 delivers for "decode_uint8_randaug") through training_step against the
    same batch augmented and resized on the host with PIL and fed as a Uint8Batch: identical patch rows, so identical loss, queue and
    gradients up to the order of the float atomics - the bounds of test_training_step_on_decoded_bytes_equals_the_host_resized_batch."""
    from tests.test_parity2_gpu import make_module
    from tests.test_path_gpu import dev_batch
    sizes = [(480, 640), (640, 480), (427, 640), (375, 500)]
    ocfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=len(sizes), adv_steps_img=2)
    batch = O.synthetic_batch(ocfg, len(sizes), 4, ragged_text=True)
    raw = raw_batch_with_plans(sizes, 11)
    res = []
    for kind in ("host", "device"):
        m, _ = make_module(ocfg, 5, "bf16", k_seed=6)
        b = dev_batch(dict(batch, image=[raw.resized_on_host().float_image()]))
        b["image"] = [raw.resized_on_host() if kind == "host" else raw]
        m.zero_grad()
        torch.manual_seed(123)                                                  # (216 patches > max_image_len: the subset is drawn on the host)
        loss = m.training_step(b, 0)
        loss.backward()
        torch.cuda.synchronize()
        res.append((float(loss), m.engine.g32.clone(), m.proj_queue.clone()))
    assert abs(res[0][0] - res[1][0]) <= 1e-6 * abs(res[0][0]) and torch.equal(res[0][2], res[1][2])
    assert float((res[0][1] - res[1][1]).norm() / res[0][1].norm()) < 1e-6
