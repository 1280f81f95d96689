"""CPU: the numpy model of the PGD threat-model kernels (tests/pgd_ball_ref.py) against plain numpy on hand cases, and its restatement
of rmcl_rng_hash against values the C function gave."""
import numpy as np
import pytest

from tests import pgd_ball_ref as R

# rmcl_rng_hash(seed, idx) of csrc/rmcl_common.h for seed in SEEDS (rows) and idx in IDX (columns).  Derivation: a host program that
# includes csrc/rmcl_common.h and prints rmcl_rng_hash(s, i) with "0x%08X" for these pairs, compiled with hipcc (the function is
# __host__ __device__ integer arithmetic, so the host's values are the device's).
SEEDS = (0, 1, 0xDEADBEEF, 12345)
IDX = (0, 1, 2, 3071, 442367, 0xFFFFFFFF)
HASH = (
    (0x00000000, 0x11FD02EB, 0xBB2AAFDE, 0xDC6FD155, 0x73EDE4A0, 0x171EE435),
    (0x514E28B7, 0xB19FEA7C, 0x0DD6B1D3, 0xFFF7DDE8, 0xA548BACC, 0x24C2350C),
    (0x0DE5C6A9, 0x331DC73E, 0xD95BCA2F, 0xCFF697FF, 0x47DEE6DA, 0x95CB1F45),
    (0x3C46C9DC, 0x9FBC9C86, 0xF8667FCA, 0x6E58C254, 0x47E73DBA, 0x7EF195C3),
)


def test_hash_matches_the_c_function():
    for s, row in zip(SEEDS, HASH):
        got = R.rng_hash(s, np.array(IDX, dtype=np.uint32))
        assert got.dtype == np.uint32 and [int(x) for x in got] == list(row), s
        assert int(R.rng_hash(s, np.uint32(IDX[3]))) == row[3]                      # scalar form


def test_start_draw_is_exact_in_fp32_and_covers_the_interval():
    v = R.start_draw(7, 3, 1 << 16)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert v.min() >= -1.0 and v.max() < 1.0 and abs(v.mean()) < 0.02 and abs((v * v).mean() - 1 / 3) < 0.02
    assert not np.array_equal(v, R.start_draw(8, 3, 1 << 16)) and not np.array_equal(v, R.start_draw(7, 4, 1 << 16))
    h = int(R.rng_hash(int(R.rng_hash(7, np.uint32(3))), np.uint32(5)))
    assert v[5] == 2 * ((h >> 8) / 2.0 ** 24) - 1


G = np.array([[3.0, -4.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
D0 = np.array([[0.5, 0.25, -0.125, 0.0], [0.5, 0.0, -0.25, 0.0]])
BASE = np.array([[0.75, -1.0, 0.0, 1.0], [0.0, 0.5, -0.5, 1.0]])


def test_directions_by_hand():
    r = R.step_ball(G, D0, 0.5, 0.0, R.DIR_NORMALISED, R.BALL_LINF)
    assert np.array_equal(r["delta"], np.array([[0.5 + 0.375, 0.25 - 0.5, -0.125, 0.125], [0.5, 0.0, -0.25, 0.0]]))
    r = R.step_ball(G, D0, 0.5, 0.0, R.DIR_SIGN, R.BALL_LINF)
    assert np.array_equal(r["delta"], np.array([[1.0, -0.25, -0.125, 0.5], [0.5, 0.0, -0.25, 0.0]]))          # sign(0) = 0
    r = R.step_ball(G, D0, 0.5, 0.0, R.DIR_L2, R.BALL_L2)
    n = np.sqrt(26.0)
    assert np.allclose(r["delta"][0], D0[0] + 0.5 * G[0] / n, rtol=0, atol=1e-15) and np.array_equal(r["delta"][1], D0[1])
    r = R.step_ball(G, D0, 0.5, 0.0, R.DIR_SIGN, R.BALL_LINF, delta_zero=True)
    assert np.array_equal(r["delta"][0], np.array([0.5, -0.5, 0.0, 0.5]))
    assert (r["allowed_delta"] >= 0).all() and np.isfinite(r["delta"]).all()


def test_projections_by_hand():
    r = R.step_ball(G, D0, 0.5, 0.75, R.DIR_SIGN, R.BALL_LINF)
    assert np.array_equal(r["delta"][0], np.array([0.75, -0.25, -0.125, 0.5]))
    t = np.array([1.0, -0.25, -0.125, 0.5])
    r = R.step_ball(G, D0, 0.5, 0.75, R.DIR_SIGN, R.BALL_L2)
    nt = np.sqrt((t * t).sum())
    assert np.allclose(r["delta"][0], t * 0.75 / nt, rtol=0, atol=1e-15) and r["scale"][0] == 0.75 / nt
    assert abs(np.sqrt((r["delta"][0] ** 2).sum()) - 0.75) < 1e-15
    assert r["scale"][1] == 1.0 and np.array_equal(r["delta"][1], D0[1])            # inside the ball: untouched
    assert (r["allowed_delta"][0] > R.step_ball(G, D0, 0.5, 0.75, R.DIR_SIGN, R.BALL_LINF)["allowed_delta"][0]).all()


def test_box_runs_after_the_ball_and_stays_inside_it():
    r = R.step_ball(G, D0, 0.5, 0.75, R.DIR_SIGN, R.BALL_LINF, base=BASE, box=(-1.0, 1.0))
    assert np.array_equal(r["x"][0], np.array([1.0, -1.0, -0.125, 1.0]))
    assert np.array_equal(r["delta"][0], np.array([0.25, 0.0, -0.125, 0.0]))
    assert (np.abs(r["delta"]) <= 0.75).all()
    nb = R.step_ball(G, D0, 0.5, 0.75, R.DIR_SIGN, R.BALL_LINF, base=BASE)
    assert np.array_equal(nb["x"][0], np.array([1.5, -1.25, -0.125, 1.5])) and np.array_equal(nb["delta"][0], np.array([0.75, -0.25, -0.125, 0.5]))
    l2, l2b = (R.step_ball(G, D0, 0.5, 0.75, R.DIR_SIGN, R.BALL_L2, base=BASE, box=b) for b in (None, (-1.0, 1.0)))
    assert (np.abs(l2b["delta"]) <= np.abs(l2["delta"])).all() and np.sqrt((l2b["delta"][0] ** 2).sum()) < 0.75
    bf = R.step_ball(G, D0, 0.5, 0.75, R.DIR_SIGN, R.BALL_L2, base=BASE, bf16_operand=True)
    assert (bf["allowed_x"] >= l2["allowed_x"] + 2.0 ** -8 * np.abs(l2["x"])).all()


def test_pad_slots_are_zero_and_take_part_in_no_norm():
    valid = [2, 0]
    r = R.step_ball(G, D0, 0.5, 0.0, R.DIR_NORMALISED, R.BALL_LINF, base=BASE, box=(-0.5, 0.5), valid=valid)
    assert np.array_equal(r["delta"][0], np.array([0.5 + 0.375, 0.25 - 0.5, 0, 0]).clip(-0.5 - BASE[0], 0.5 - BASE[0]) * [1, 1, 0, 0])
    assert np.array_equal(r["delta"][1], np.zeros(4)) and np.array_equal(r["x"][1], BASE[1])               # all pad: base, unboxed
    assert np.array_equal(r["x"][0, 2:], BASE[0, 2:]) and (r["allowed_delta"][~r["mask"]] == 0).all()
    g2 = G.copy()
    g2[0, 3] = 100.0                                                                                        # a pad element's gradient
    r2 = R.step_ball(g2, D0, 0.5, 0.0, R.DIR_L2, R.BALL_L2, valid=valid)
    assert np.allclose(r2["delta"][0, :2], D0[0, :2] + 0.5 * G[0, :2] / 5.0, rtol=0, atol=1e-15)


def test_random_start_by_hand():
    v = np.stack([R.start_draw(9, 2 + b, 8) for b in range(2)])
    r = R.random_start(2, 8, 2, 9, 0.25, R.BALL_LINF)
    assert np.array_equal(r["delta"], 0.25 * v)
    d32, x32 = R.random_start_linf_f32(2, 8, 2, 9, 0.25)
    assert x32 is None and np.array_equal(d32.astype(np.float64), r["delta"])
    r = R.random_start(2, 8, 2, 9, 0.25, R.BALL_L2, valid=[8, 4])
    assert np.allclose(np.sqrt((r["delta"] ** 2).sum(axis=1)), 0.25, rtol=1e-15) and (r["delta"][1, 4:] == 0).all()
    assert np.allclose(r["delta"][1, :4], 0.25 * v[1, :4] / np.sqrt((v[1, :4] ** 2).sum()), rtol=1e-15)
    whole = R.random_start(4, 8, 0, 9, 0.25, R.BALL_LINF)["delta"]
    halves = np.concatenate([R.random_start(2, 8, s0, 9, 0.25, R.BALL_LINF)["delta"] for s0 in (0, 2)])
    assert np.array_equal(whole, halves)
    base = np.full((2, 8), 0.9, dtype=np.float32)
    d32, x32 = R.random_start_linf_f32(2, 8, 2, 9, 0.25, base=base, box=(-1.0, 1.0))
    assert x32.max() <= 1.0 and (x32 == 1.0).any() and np.array_equal(d32, x32 - base)


@pytest.mark.parametrize("G_", [1, 2])
def test_keep_worst_by_hand(G_):
    nan = np.float32("nan")
    delta = np.arange(4 * G_ * 4, dtype=np.float32).reshape(4 * G_, 4)
    best = -np.ones_like(delta)
    bs, br, bd, _, take = R.keep_worst([1.0, nan, 3.0, 2.0], np.zeros(4, np.float32), np.full(4, 9, np.int32), 0, G_, delta, best)
    assert take.all() and np.array_equal(bd, delta) and (br == 0).all() and np.isnan(bs[1])                  # restart 0 takes everything
    bs2, br2, bd2, _, take = R.keep_worst([1.0, 5.0, nan, 2.5], bs, br, 1, G_, best, bd)
    assert list(take) == [False, False, False, True]                # tie, NaN best (5 > NaN is false), NaN score, strictly larger
    assert list(br2) == [0, 0, 0, 1] and bs2[3] == 2.5 and bs2[0] == 1.0
    assert np.array_equal(bd2[: 3 * G_], delta[: 3 * G_]) and (bd2[3 * G_:] == -1).all()
