"""CPU: the numpy statements of tests/align_ref.py - the NEAREST tables against PIL itself, the float64 heat model against the demo's
arithmetic, the float32 restatement of the IPOT kernel's summation order against the float64 oracle - the fixture
tests/golden/align_L2.npz against the float64 model, the engine's host-side table builder, and (hipcc cross-compiles gfx950 without a
GPU) the scratch use of the kernels of csrc/align.hip."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import rmcl_pkg  # noqa: F401
from rmcl_amd.runtime import Engine
from oracle import rmcl_oracle as O
from tests import align_fixture as AF
from tests import align_ref as R
from tests.golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc", "align.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]
KERNELS = ("ipot_plan_kernelILi1E", "ipot_plan_kernelILi2E", "align_heat_kernel")          # one and two plan rows per thread
# (source H, W) -> (Hout, Wout); the third is the case where the closed form misses, the last two shrink
RESIZES = [((12, 12), (384, 384)), ((3, 4), (96, 128)), ((12, 19), (333, 500)), ((1, 1), (7, 5)), ((24, 24), (7, 5)), ((12, 20), (8, 30)),
           ((18, 12), (571, 383))]


@pytest.mark.parametrize("src,dst", RESIZES)
def test_nearest_tables_are_pils(src, dst):
    (H, W), (Ho, Wo) = src, dst
    cells = np.arange(H * W, dtype=np.int32).reshape(H, W)
    want = np.array(Image.fromarray(cells, "I").resize((Wo, Ho), resample=Image.NEAREST))
    ty, tx = R.nearest_table(H, Ho), R.nearest_table(W, Wo)
    assert np.array_equal(cells[ty][:, tx], want)
    assert Engine.nearest_table(H, Ho) == ty.tolist() and Engine.nearest_table(W, Wo) == tx.tolist()      # the engine's host builder
    by = (cells % 256).astype(np.uint8)
    heat = by.astype(np.float64) / 255.0
    assert np.array_equal(R.alpha_bytes(heat, Ho, Wo), np.array(Image.fromarray(by, "L").resize((Wo, Ho), resample=Image.NEAREST)))


def test_the_closed_form_is_not_pils():
    cells = np.arange(12 * 19, dtype=np.int32).reshape(12, 19)
    want = np.array(Image.fromarray(cells, "I").resize((500, 333), resample=Image.NEAREST))
    closed = cells[R.nearest_table_closed_form(12, 333)][:, R.nearest_table_closed_form(19, 500)]
    assert int((closed != want).sum()) > 0


def demo_heat64(g):
    """demo.py:141-143 in torch float64 (torch's std is the unbiased one)"""
    h = torch.from_numpy(np.asarray(g, dtype=np.float64))
    h = (h - h.mean()) / h.std()
    h = torch.clamp(h, 1.0, 3.0)
    return ((h - h.min()) / (h.max() - h.min())).numpy()


def test_heat_model_is_the_demos_arithmetic_and_marks_its_nans():
    rng = np.random.RandomState(3)
    for H, W in ((3, 4), (12, 20), (1, 2), (4, 4)):
        g = rng.rand(H, W) ** 6
        heat, flat = R.heat_one(g)
        ref = demo_heat64(g)
        if flat:
            assert np.isnan(ref).all() and (heat == 0).all()
        else:
            assert np.abs(heat - ref).max() <= R.heat_allowance(g)
            assert heat.min() == 0.0 and heat.max() == 1.0
            assert np.array_equal(R.heat_one(7.0 * g)[0] > 0, heat > 0)                     # the demo's factor len(txt_emb) cancels
    for g, valid in ((np.zeros((3, 4)), True), (np.full((3, 4), 0.25), True), (np.array([[0.5]]), True), (np.array([[0.1, 0.9]]), True),
                     (rng.rand(3, 4), False)):
        heat, flat = R.heat_one(g, valid)
        assert flat == 1 and (heat == 0).all()
        if valid:
            with np.errstate(all="ignore"):
                assert np.isnan(demo_heat64(g)).all()
    grid = rng.rand(2, 3, 2, 5)
    heat, flat = R.heat_model(grid, np.array([[1, 0, 1], [0, 1, 1]]))
    assert flat.tolist() == [[0, 1, 0], [1, 0, 0]] and (heat[0, 1] == 0).all() and np.array_equal(heat[1, 2], R.heat_one(grid[1, 2])[0])


def test_scatter_drops_the_cls_row_and_out_of_grid_slots():
    T = np.arange(2 * 4 * 3, dtype=np.float32).reshape(2, 4, 3) + 1
    grid = R.scatter(T, np.array([[5, 0, -1], [2, 6, 1]]), 2, 3)
    assert grid.shape == (2, 3, 2, 3)
    assert grid[0, 1].reshape(-1).tolist() == [T[0, 2, 1], 0, 0, 0, 0, T[0, 1, 1]]
    assert grid[1, 2].reshape(-1).tolist() == [0, T[1, 3, 2], T[1, 1, 2], 0, 0, 0]


def masks(B, Lt, Li, seed):
    rng = np.random.RandomState(seed)
    tv = (rng.rand(B, Lt) < 0.7).astype(np.int32)
    iv = (rng.rand(B, Li) < 0.8).astype(np.int32)
    tv[0], iv[1] = 0, 1
    tv[1] = 1
    if B > 2:
        iv[2], iv[2, Li // 2] = 0, 1
        tv[2, 0] = 1
    return tv, iv


@pytest.mark.parametrize("Lt,Li,iters,beta", [(7, 65, 50, 0.5), (40, 145, 50, 0.5), (5, 300, 50, 0.5), (12, 13, 1000, 0.1), (1, 1, 3, 0.5)])
def test_the_fp32_restatement_against_the_fp64_oracle(Lt, Li, iters, beta):
    """the rule of tests/test_wpa_kernels_gpu.py: allowed = 8 * max(e32, 2^-23 max T), e32 the fp32 oracle's own distance from the fp64 one"""
    B = 3
    g = torch.Generator().manual_seed(Lt * Li)
    xt = torch.nn.functional.normalize(torch.randn(B, Lt, 768, generator=g), dim=-1)
    xi = torch.nn.functional.normalize(torch.randn(B, Li, 768, generator=g), dim=-1)
    tv, iv = masks(B, Lt, Li, seed=Lt + Li)
    tvt, ivt = torch.from_numpy(tv), torch.from_numpy(iv)
    jp = (tvt[:, :, None] == 0) | (ivt[:, None, :] == 0)
    cost = (1.0 - xt @ xi.transpose(1, 2)).masked_fill(jp, 0.0)
    T = R.ipot_plan_f32(cost.numpy(), tv, iv, beta, iters)

    def oracle(dt):
        with np.errstate(all="ignore"):
            return O.ipot(cost.to(dt), tvt.sum(1).to(dt), tvt == 0, ivt.sum(1).to(dt), ivt == 0, jp, beta, iters, 1)

    T64, T32 = oracle(torch.float64), oracle(torch.float32)
    assert np.isfinite(T).all()
    assert (T[jp.transpose(1, 2).numpy()] == 0).all() and (T[0] == 0).all()
    base = max(float((T32.double() - T64).abs().max()), 2.0 ** -23 * float(T64.max()))
    dev = float(np.abs(T.astype(np.float64) - T64.numpy()).max())
    print("restatement", (Lt, Li, iters), "dev / base", dev / base)
    assert dev <= 8.0 * base
    live = (tv.sum(1) > 0) & (iv.sum(1) > 0)
    assert np.abs(T.astype(np.float64).sum((1, 2))[live] - 1).max() <= 1e-5


@pytest.mark.parametrize("case", list(AF.CASES))
def test_the_fixture_against_the_float64_model(case):
    g = load(AF.FIXTURE)
    H, W = (int(v) for v in g[f"{case}_grid_hw"])
    cells, tv = g[f"{case}_cells"], g[f"{case}_txt_valid"]
    batch = AF.make_batch(AF.config(), case)
    assert np.array_equal(batch["text_ids"].numpy(), g[f"{case}_ids"]) and np.array_equal(batch["text_masks"].numpy(), g[f"{case}_masks"])
    t_valid, _ = AF.demo_masks(g[f"{case}_masks"], np.ones((tv.shape[0], 1)))
    assert np.array_equal(t_valid.numpy(), tv)
    # the cost is the cosine cost of the stored features under the stored masks
    tf, imf = torch.from_numpy(g[f"{case}_text_feats"]).double(), torch.from_numpy(g[f"{case}_image_feats"]).double()
    c64 = 1 - torch.nn.functional.normalize(tf, dim=-1, eps=1e-5) @ torch.nn.functional.normalize(imf, dim=-1, eps=1e-5).transpose(1, 2)
    jp = torch.from_numpy(~tv[:, :, None] | ~g[f"{case}_img_valid"][:, None, :])
    assert float((c64.masked_fill(jp, 0) - torch.from_numpy(g[f"{case}_cost"]).double()).abs().max()) <= 1e-6
    for t in AF.ITERS:
        plan = g[f"{case}_plan_{t}"]
        grid = R.scatter(plan.astype(np.float64), cells, H, W)
        heat, flat = R.heat_model(grid, tv)
        assert np.array_equal(flat, g[f"{case}_flat_{t}"])
        ref = g[f"{case}_heat_{t}"].astype(np.float64)
        # the demo computes in fp32: about H W roundings in mean and std, amplified by 1 / (max - min) of the clipped values
        for b, m in zip(*np.nonzero(flat == 0)):
            gm = grid[b, m]
            c = np.clip((gm - gm.mean()) / gm.std(ddof=1), 1, 3)
            tol = 4 * (H * W + 8) * 2.0 ** -24 * (1 + abs(gm.mean()) / gm.std(ddof=1)) * 3 / (c.max() - c.min())
            assert np.abs(heat[b, m] - ref[b, m]).max() <= tol, (case, t, b, m)
            assert np.array_equal(heat[b, m] > 0, ref[b, m] > 0) and int(heat[b, m].argmax()) == int(ref[b, m].argmax())
            ok = g[f"{case}_byte_ok_{t}"][b, m]
            assert np.array_equal(R.alpha_bytes(heat[b, m], H, W)[ok], g[f"{case}_bytes_{t}"][b, m][ok])
        assert (ref[flat == 1] == 0).all()
    tok = g[f"{case}_token"]
    t = AF.ITERS[-1]
    alpha = g[f"{case}_alpha_{t}"]
    for b in range(tv.shape[0]):
        assert flat[b, tok[b]] == 0
        assert np.array_equal(alpha[b], R.alpha_bytes(g[f"{case}_heat_{t}"][b, tok[b]], *alpha.shape[1:]))


@pytest.fixture(scope="module")
def isa():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "align.s")
        r = subprocess.run(["hipcc", *FLAGS, SRC, "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(dst).read()


def test_align_kernels_are_present_and_use_no_scratch(isa):
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    names = " ".join(n for n, _ in sizes)
    for k in KERNELS:
        assert k in names, k
    spilled = [(n[:80], int(s)) for n, s in sizes if int(s) != 0]
    assert not spilled, spilled
