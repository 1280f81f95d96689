"""-m gpu: masked patch prediction on the byte feed.

Kernel: rmcl_mpp_labels_u8 (csrc/mpp.hip) writes, integer for integer, what rmcl_mpp_labels writes for ``Uint8Batch.float_image()`` of
the same bytes - dense and selected form, ragged extents (a fully padded patch of the dense form: 127), every byte value, garbage in the
padding, guard words behind the output, a second call, rejected calls - and stands to the oracle's labels (tests/mpp_oracle.py) as the
float kernel does in tests/test_mpp_kernels_gpu.py.

Pass: compute_mpp, infer(mask_image=True) and visual_embed(mask_it=True) on a ``Uint8Batch`` / ``RawUint8Batch`` against the same call on
the float batch.  The rule between the byte feed and the float feed is the one of tests/test_feed_gpu.py
(test_training_step_on_a_byte_batch_equals_the_float_batch): identical patch rows in, so |loss_a - loss_b| <= 1e-6 |loss_a| and
||g_a - g_b|| / ||g_a|| < 1e-6 over the gradient arena (the order of its float atomics); the labels are integers and must be equal."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd._lib import lib, check, P  # noqa: E402
from rmcl_amd.runtime import stream_ptr  # noqa: E402
from rmcl_amd.vilt.datasets import RawUint8Batch, Uint8Batch, select_from_sizes  # noqa: E402
from rmcl_amd.vilt.transforms import normalize_lut  # noqa: E402
from tests import mpp_oracle as M  # noqa: E402
from tests.test_mpp_gpu import _step, make_module, with_masks  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"
C = ctypes
GUARD = 16


def byte_batch(sizes, Hmax, Wmax, seed, garbage=False):
    g = torch.Generator().manual_seed(seed)
    data = torch.zeros(len(sizes), Hmax, Wmax, 3, dtype=torch.uint8)
    if garbage:                                                          # non-zero bytes outside every sample: must never be read as pixels
        data = torch.randint(1, 256, data.shape, generator=torch.Generator().manual_seed(seed + 1000), dtype=torch.uint8)
    for b, (h, w) in enumerate(sizes):
        data[b, :h, :w] = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    return Uint8Batch(data, torch.tensor(sizes, dtype=torch.int32))


def ragged_sizes(B, Hmax, Wmax, seed):
    """sample 0 fills the batch; the others take seeded multiples of 32 (fully padded patches wherever the grid allows them)"""
    g = torch.Generator().manual_seed(seed)
    out = [(Hmax, Wmax)]
    for _ in range(B - 1):
        out.append((32 * int(torch.randint(1, Hmax // 32 + 1, (1,), generator=g)), 32 * int(torch.randint(1, Wmax // 32 + 1, (1,), generator=g))))
    return out


def labels_float(img, sel=None, counts=None, Pn=None):
    B, _, H, W = img.shape
    Pn = (H // 32) * (W // 32) if Pn is None else Pn
    out = torch.full((B, Pn, 3), -7, dtype=torch.int32, device=DEV)
    d = img.to(DEV).contiguous()
    if sel is None:
        check(lib.rmcl_mpp_labels(P(d), B, H, W, None, None, 0, W // 32, Pn, P(out), stream_ptr()))
    else:
        s, c = sel.to(DEV, torch.int32).contiguous(), counts.to(DEV, torch.int32).contiguous()
        check(lib.rmcl_mpp_labels(P(d), B, H, W, P(s), P(c), s.shape[1], W // 32, Pn, P(out), stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().long()


def labels_u8(u8, sel=None, counts=None, Pn=None, data=None):
    """rmcl_mpp_labels_u8 into a buffer with GUARD words behind it (checked here), called twice (the outputs must be identical)"""
    B, _, H, W = u8.shape
    Pn = (H // 32) * (W // 32) if Pn is None else Pn
    d = (u8.data if data is None else data).to(DEV).contiguous()
    sz, lut = u8.sizes.to(DEV).contiguous(), normalize_lut().to(DEV)
    outs = []
    for _ in range(2):
        buf = torch.full((B * Pn * 3 + GUARD,), -7, dtype=torch.int32, device=DEV)
        if sel is None:
            check(lib.rmcl_mpp_labels_u8(P(d), P(sz), B, H, W, P(lut), None, None, 0, W // 32, Pn, P(buf), stream_ptr()))
        else:
            s, c = sel.to(DEV, torch.int32).contiguous(), counts.to(DEV, torch.int32).contiguous()
            check(lib.rmcl_mpp_labels_u8(P(d), P(sz), B, H, W, P(lut), P(s), P(c), s.shape[1], W // 32, Pn, P(buf), stream_ptr()))
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[B * Pn * 3:] == -7).all()), "guard words behind the labels were written"
        outs.append(host[: B * Pn * 3].view(B, Pn, 3).long())
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def constant_label(c):
    """the label of a patch whose bytes are all c: 1024 equal addends sum exactly in every order, so the kernel's value is
    ((lut[c] * 0.5 + 0.5) * 255) in fp32 (x * 0.5 is exact: one rounding in the add, one in the product), truncated"""
    x = normalize_lut()[torch.as_tensor(c).long()] * 0.5 + 0.5
    return (x * 255.0).long()


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("Hmax,Wmax", [(32, 32), (64, 96), (96, 64)])
def test_labels_equal_the_float_kernel_on_the_float_image(Hmax, Wmax, B):
    """B * P on both sides of a multiple of 4 (four slots per workgroup): P = 1 and 6, B = 1, 2, 3, 5"""
    sizes = ragged_sizes(B, Hmax, Wmax, 10 * B + Hmax)
    u8 = byte_batch(sizes, Hmax, Wmax, 3 + B)
    img = u8.float_image()
    gh, gw = Hmax // 32, Wmax // 32
    want = labels_float(img)
    got = labels_u8(u8)
    assert torch.equal(got, want)
    for b, (h, w) in enumerate(sizes):                                    # the dense form: a fully padded patch is 0 * 0.5 + 0.5 -> 127
        for q in range(gh * gw):
            if q // gw >= h // 32 or q % gw >= w // 32:
                assert got[b, q].tolist() == [127, 127, 127], (b, q)
    # garbage bytes in the padding change no label
    assert torch.equal(labels_u8(byte_batch(sizes, Hmax, Wmax, 3 + B, garbage=True)), want)
    # the selected form, with the selection of the batch's own extents
    sel, counts, _ = select_from_sizes(u8.sizes, gh, gw)
    n = int(counts.max())
    got_s = labels_u8(u8, sel, counts, Pn=n)
    assert torch.equal(got_s, labels_float(img, sel, counts, Pn=n))
    for b in range(B):
        assert bool((got_s[b, int(counts[b]):] == -100).all()) and bool((got_s[b, : int(counts[b])] >= 0).all())
    assert torch.equal(labels_u8(byte_batch(sizes, Hmax, Wmax, 3 + B, garbage=True), sel, counts, Pn=n), got_s)


def test_ragged_extents_inside_64_by_96():
    sizes = [(32, 64), (64, 32), (64, 96)]
    u8 = byte_batch(sizes, 64, 96, 21, garbage=True)
    got = labels_u8(u8)
    assert torch.equal(got, labels_float(u8.float_image()))
    assert bool((got[0, [2, 3, 4, 5]] == 127).all()) and bool((got[1, [1, 2, 4, 5]] == 127).all())


def test_selected_form_counts_zero_one_and_sel_ld():
    """counts 0 and 1, a slot count P above sel_ld, a patch index outside the grid: -100 in all three channels"""
    u8 = byte_batch([(64, 96), (64, 96), (32, 64), (64, 96)], 64, 96, 22)
    img = u8.float_image()
    sel = torch.tensor([[5, 4], [3, 0], [1, 0], [7, 2]], dtype=torch.int32)      # sel_ld = 2; sample 3's first index lies outside the 2 x 3 grid
    counts = torch.tensor([0, 1, 2, 2], dtype=torch.int32)
    got = labels_u8(u8, sel, counts, Pn=3)
    assert torch.equal(got, labels_float(img, sel, counts, Pn=3))
    full = labels_float(img)
    assert bool((got[0] == -100).all())
    assert torch.equal(got[1, 0], full[1, 3]) and bool((got[1, 1:] == -100).all())
    assert torch.equal(got[2, 0], full[2, 1]) and torch.equal(got[2, 1], full[2, 0]) and bool((got[2, 2] == -100).all())
    assert bool((got[3, 0] == -100).all()) and torch.equal(got[3, 1], full[3, 2]) and bool((got[3, 2] == -100).all())


def test_every_byte_value_and_distinct_channels():
    """a constant c per patch for every c in 0..255 (every truncation boundary), all 0 / all 255, and patches whose three channels differ
    (a mix-up of the channels inside the 12-byte read would move them)"""
    data = torch.zeros(1, 512, 512, 3, dtype=torch.uint8)                # 16 x 16 = 256 patches
    for c in range(256):
        data[0, (c // 16) * 32:(c // 16) * 32 + 32, (c % 16) * 32:(c % 16) * 32 + 32] = c
    u8 = Uint8Batch(data, torch.tensor([[512, 512]], dtype=torch.int32))
    got = labels_u8(u8)
    assert torch.equal(got, labels_float(u8.float_image()))
    want = constant_label(torch.arange(256))
    assert torch.equal(got[0], want[:, None].expand(256, 3))
    assert got[0, 0].tolist() == [0, 0, 0] and got[0, 255].tolist() == [255, 255, 255]
    assert bool(((want - torch.arange(256)).abs() <= 1).all())           # (the fp32 formula lands on c or next to it)
    chan = torch.tensor([[10, 100, 200], [255, 0, 128], [1, 2, 3]], dtype=torch.uint8)
    d2 = torch.zeros(3, 32, 32, 3, dtype=torch.uint8)
    for b in range(3):
        d2[b] = chan[b]
    u2 = Uint8Batch(d2, torch.tensor([[32, 32]] * 3, dtype=torch.int32))
    g2 = labels_u8(u2)
    assert torch.equal(g2, labels_float(u2.float_image()))
    assert torch.equal(g2[:, 0], constant_label(chan))
    assert g2[1, 0].tolist()[:2] == [255, 0]
    # ... and channels that differ pixel by pixel inside one patch
    d3 = torch.zeros(1, 32, 32, 3, dtype=torch.uint8)
    d3[0, :, :, 0] = torch.arange(32, dtype=torch.uint8)[None, :] * 8
    d3[0, :, :, 1] = torch.arange(32, dtype=torch.uint8)[:, None] * 3
    d3[0, :, :, 2] = 250
    u3 = Uint8Batch(d3, torch.tensor([[32, 32]], dtype=torch.int32))
    g3 = labels_u8(u3)
    assert torch.equal(g3, labels_float(u3.float_image())) and len(set(g3[0, 0].tolist())) == 3


def test_labels_stand_to_the_oracle_as_the_float_kernel_does():
    """tests/test_mpp_kernels_gpu.py::test_labels_generic_float_pixels on bytes: equal to floor(fp64 mean * 255) outside a band of 1e-3
    around the integers, within one of it inside; and tests/test_mpp_gpu.py's comparison with the oracle's image_labels under that rule"""
    sizes = [(96, 96), (64, 96), (96, 32), (32, 32)]
    u8 = byte_batch(sizes, 96, 96, 23)
    img = u8.float_image()
    v = M.patch_means_fp64(img)
    band = (v - v.round()).abs() < 1e-3
    got = labels_u8(u8)
    assert torch.equal(got[~band], v.floor().long()[~band])
    assert bool(((got - v.floor().long()).abs() <= 1)[band].all())
    ref32 = M.patch_labels(img)
    assert torch.equal(ref32[~band], got[~band])
    cfg = O.default_config(max_image_len=-1)
    masked, _ = M.make_masks(img, cfg, 5)
    sel, counts, _ = select_from_sizes(u8.sizes, 3, 3)
    n = int(counts.max())
    lab = labels_u8(u8, sel, counts, Pn=n)
    mk = torch.gather(masked, 1, sel[:, :n].long())
    mine = torch.where(mk.unsqueeze(-1), lab, torch.full_like(lab, -100))
    mine[lab == -100] = -100
    want = M.image_labels(img, cfg, masked)[:, 1:]
    vs = torch.gather(v, 1, sel[:, :n].long().unsqueeze(-1).expand(-1, -1, 3))
    bs = (vs - vs.round()).abs() < 1e-3
    assert tuple(want.shape) == tuple(mine.shape)
    assert torch.equal((want == -100), (mine == -100))
    assert torch.equal(mine[~bs], want[~bs]) and bool(((mine - want).abs() <= 1).all())


def test_bad_calls_are_rejected_before_any_launch():
    buf = (C.c_uint8 * 64)()
    fb = (C.c_float * 256)()
    ib = (C.c_int32 * 16)()

    def rejected(rc):
        msg = lib.rmcl_last_error()
        assert rc == -1 and msg and b"mpp_labels_u8" in msg, (rc, msg)

    rejected(lib.rmcl_mpp_labels_u8(None, ib, 1, 32, 32, fb, None, None, 0, 1, 1, ib, None))
    rejected(lib.rmcl_mpp_labels_u8(buf, None, 1, 32, 32, fb, None, None, 0, 1, 1, ib, None))          # NULL sizes
    rejected(lib.rmcl_mpp_labels_u8(buf, ib, 1, 32, 32, None, None, None, 0, 1, 1, ib, None))          # NULL lut
    rejected(lib.rmcl_mpp_labels_u8(buf, ib, 1, 32, 32, fb, None, None, 0, 1, 1, None, None))
    rejected(lib.rmcl_mpp_labels_u8(buf, ib, 1, 32, 32, fb, ib, None, 1, 1, 1, ib, None))              # sel without counts
    rejected(lib.rmcl_mpp_labels_u8(buf, ib, 1, 48, 32, fb, None, None, 0, 1, 1, ib, None))            # Hmax % 32 != 0
    rejected(lib.rmcl_mpp_labels_u8(buf, ib, 1, 32, 48, fb, None, None, 0, 1, 1, ib, None))
    rejected(lib.rmcl_mpp_labels_u8(buf, ib, 1, 64, 64, fb, None, None, 0, 2, 3, ib, None))            # dense P != gh * gw
    rejected(lib.rmcl_mpp_labels_u8(buf, ib, 1, 64, 64, fb, ib, ib, 4, 3, 4, ib, None))                # gw != Wmax / 32


# ---- the pass ------------------------------------------------------------------------------------------------------------------------
RAGGED = ([(96, 128), (64, 96), (128, 96), (32, 64)], 128, 128)
FULL = ([(384, 384)] * 2, 384, 384)


def _case(sizes, Hmax, Wmax, seed):
    B = len(sizes)
    cfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=B, max_image_len=-1)
    p = dict(O.init_params(cfg, 3), **M.mpp_init_params(cfg, 4))
    u8 = byte_batch(sizes, Hmax, Wmax, seed)
    img = u8.float_image()
    batch = dict(O.synthetic_batch(cfg, B, 5, ragged_text=True), image=[img])
    masked, replaced = M.make_masks(img, cfg, 7, "ragged" if B >= 4 else "random")
    return cfg, p, u8, batch, masked, replaced


def _mpp_step(cfg, p, batch, image, masked, replaced):
    """one training step of a model whose only task is mpp (training_step -> objectives.compute_mpp), then the labels of a second forward"""
    m = make_module(cfg, p, "f32", max_image_len=-1)
    db = with_masks(dev_batch(batch), masked, replaced)
    db["image"] = [image]
    torch.manual_seed(31)
    _step(m, db)
    assert set(m.current_tasks) == {"mpp"}
    loss, grads = float(m.logged["mpp/train/loss"]), m.engine.g32.clone()
    labels = m(db)["mpp_labels"].cpu()
    return loss, labels, grads, m, db


@pytest.mark.parametrize("shape", [RAGGED, FULL], ids=["ragged_128", "dense_384"])
def test_compute_mpp_on_bytes_equals_the_float_batch(shape):
    cfg, p, u8, batch, masked, replaced = _case(*shape, seed=41)
    lf, labf, gf, _, _ = _mpp_step(cfg, p, batch, batch["image"][0], masked, replaced)
    lb, labb, gb, m, db = _mpp_step(cfg, p, batch, u8, masked, replaced)
    assert int((labf != -100).sum()) > 0
    assert torch.equal(labb, labf)
    print("mpp_loss float", lf, "bytes", lb, "grad rel", float((gf - gb).norm() / gf.norm()))
    assert abs(lf - lb) <= 1e-6 * abs(lf)
    assert float((gf - gb).norm() / gf.norm()) < 1e-6
    # infer(mask_image=True) and visual_embed(mask_it=True): bytes against float, on the model of the byte step
    with torch.no_grad():
        ob = m.infer(db, mask_image=True)
        of = m.infer(dict(db, image=[batch["image"][0].to(DEV)]), mask_image=True)
        vb = m.visual_embed(u8, max_image_len=-1, mask_it=True, mpp_masks=(masked, replaced))
        vf = m.visual_embed(batch["image"][0].to(DEV), max_image_len=-1, mask_it=True, mpp_masks=(masked, replaced))
    assert torch.equal(ob["image_labels"], of["image_labels"]) and torch.equal(ob["image_labels"].cpu(), labf)
    assert torch.equal(ob["image_masks"], of["image_masks"])
    for k in ("text_feats", "image_feats", "cls_feats", "raw_cls_feats"):
        assert float((ob[k] - of[k]).abs().max()) <= 1e-6 * max(1.0, float(of[k].abs().max())), k
    assert torch.equal(vb[3], vf[3]) and torch.equal(vb[1], vf[1]) and torch.equal(vb[2][0].cpu(), vf[2][0].cpu()) and vb[2][1] == vf[2][1]
    assert float((vb[0] - vf[0]).abs().max()) <= 1e-6 * max(1.0, float(vf[0].abs().max()))


def test_compute_mpp_from_decoded_bytes_equals_the_host_resized_batch():
    """a RawUint8Batch (decoded, MinMaxResize owed) goes through the device resize; against the float image of the PIL-resized bytes"""
    g = torch.Generator().manual_seed(51)
    sizes = [(60, 80), (80, 60), (64, 64), (50, 90)]
    data = torch.zeros(4, 80, 90, 3, dtype=torch.uint8)
    for b, (h, w) in enumerate(sizes):
        data[b, :h, :w] = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    raw = RawUint8Batch(data, torch.tensor(sizes, dtype=torch.int32), 96, 160)
    host = raw.resized_on_host()
    cfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=4, max_image_len=-1)
    p = dict(O.init_params(cfg, 3), **M.mpp_init_params(cfg, 4))
    img = host.float_image()
    batch = dict(O.synthetic_batch(cfg, 4, 5, ragged_text=True), image=[img])
    masked, replaced = M.make_masks(img, cfg, 7, "ragged")
    assert tuple(raw.shape) == tuple(img.shape)                           # G and the mask draws come from the batch's shape
    lf, labf, gf, _, _ = _mpp_step(cfg, p, batch, img, masked, replaced)
    lb, labb, gb, _, _ = _mpp_step(cfg, p, batch, raw, masked, replaced)
    assert torch.equal(labb, labf) and int((labf != -100).sum()) > 0
    assert abs(lf - lb) <= 1e-6 * abs(lf) and float((gf - gb).norm() / gf.norm()) < 1e-6


def test_mask_draws_on_bytes_follow_the_float_batch():
    """without injected masks both feeds draw from torch's CPU generator in the same order: equal image_labels under one seed"""
    cfg, p, u8, batch, _, _ = _case(*RAGGED, seed=43)
    m = make_module(cfg, p, "f32", max_image_len=-1)
    db = dev_batch(batch)
    out = []
    for image in (db["image"][0], u8):
        torch.manual_seed(11)
        with torch.no_grad():
            out.append(m.infer(dict(db, image=[image]), mask_image=True)["image_labels"])
    assert torch.equal(out[0], out[1]) and int((out[0] != -100).sum()) > 0


def test_sizes_are_validated_on_the_host():
    cfg, p, u8, batch, masked, replaced = _case(*RAGGED, seed=44)
    m = make_module(cfg, p, "f32", max_image_len=-1)
    bad = Uint8Batch(u8.data, torch.tensor([[96, 128], [64, 96], [160, 96], [32, 64]], dtype=torch.int32))   # h above the padded batch
    db = with_masks(dev_batch(batch), masked, replaced)
    db["image"] = [bad]
    with pytest.raises(ValueError, match="sizes"):
        with torch.no_grad():
            m.infer(db, mask_image=True)
