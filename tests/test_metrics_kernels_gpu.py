"""-m gpu: rmcl_metrics_update (csrc/metrics.hip) through the C ABI against the float64 / integer statement of tests/metrics_ref.py.

Counts are exact.  A sum is compared with math.fsum of the exact double values of its fp32 addends: the kernel adds the same addends in
double, so ANY order stays within ``n * 2^-53 * sum|x|``, n = addends into the slot so far (the rule of
tests/test_guarded_step_kernels_gpu.py).  The shapes are the ones at which the kernel changes arm: rows around the wave (64) and the
workgroup (256) and into the strided loop (1000), columns around the wave's 64 lanes and the VQA head's 3129 at a pitch with garbage in
the pad columns.  The table sits between guard bytes.  The largest |error| / bound goes to the file named by RMCL_METRICS_PARITY_OUT when
set (profiles/epoch_metrics_parity.json is such a dump)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, stream  # noqa: E402
from tests import metrics_ref as R  # noqa: E402

GUARD, SENTINEL = 256, 0xA5
N_SLOTS = 24
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
NCOLS = [1, 2, 3, 63, 64, 65, 3129]
PARITY = {"largest_ratio": 0.0, "where": None, "checked_sums": 0}


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_METRICS_PARITY_OUT")
    if out and PARITY["checked_sums"]:
        with open(out, "w") as f:
            json.dump({"rule": "|sum - fsum| <= addends * 2^-53 * sum|x|; counts exact", **PARITY}, f, indent=1, sort_keys=True)


class Table:
    """the device table between guard bytes, and the reference next to it"""

    def __init__(self, n_slots=N_SLOTS):
        self.buf = torch.full((2 * GUARD + 16 * n_slots,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.buf[GUARD:GUARD + 16 * n_slots].view(torch.float64).view(n_slots, 2)
        self.t.zero_()
        self.ref = R.RefTable(n_slots)
        self.n_slots = n_slots
        self.keep = []

    def dev(self, a, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)
        self.keep.append(t)
        return t

    def call(self, ops):
        """ops: dicts of metrics_ref.apply keywords (numpy inputs) + kind / slot; launches them as ONE rmcl_metrics_update"""
        packed = L.MetricOps(n_ops=len(ops))
        for i, o in enumerate(ops):
            o = dict(o)
            f = dict(kind=o["kind"], slot=o["slot"], n_groups=o.get("n_groups", 1), flags=o.get("flags", 0), rows=o.get("rows", 0),
                     stride=o.get("stride", 1), ignore_index=o.get("ignore_index", -100), scale=o.get("scale", 1.0), imm=o.get("imm", 0.0))
            a, b, g = o.get("a"), o.get("b"), o.get("group")
            int_a = o["kind"] == R.MATCH
            if a is not None:
                f["a"] = self.dev(a, torch.int32 if int_a else torch.float32).data_ptr()
            if b is not None:
                f["b"] = self.dev(b, torch.float32 if o["kind"] in (R.PAIR, R.SCALAR) else torch.int32).data_ptr()
            if g is not None:
                f["group"] = self.dev(g, torch.int32).data_ptr()
            if o["kind"] == R.ARGMAX_MATCH:
                f["ncols"], f["pitch"] = o["ncols"], np.asarray(a).shape[1]
            packed.op[i] = L.MetricOp(**f)
            R.apply(self.ref, **o)
        return lib.rmcl_metrics_update(self.t.data_ptr(), self.n_slots, C.byref(packed), stream())

    def check(self, where):
        torch.cuda.synchronize()
        got = self.t.cpu().numpy()
        raw = self.buf.cpu()
        assert bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[-GUARD:] == SENTINEL).all()), f"{where}: guard bytes written"
        for s in range(self.n_slots):
            assert got[s, 1] == self.ref.t[s, 1], (where, s, got[s], self.ref.t[s])                    # counts: exact
            err, bound = abs(got[s, 0] - self.ref.t[s, 0]), self.ref.bound(s)
            assert err <= bound, (where, s, got[s, 0], self.ref.t[s, 0], err, bound)
            if bound > 0:
                PARITY["checked_sums"] += 1
                if err / bound > PARITY["largest_ratio"]:
                    PARITY["largest_ratio"], PARITY["where"] = err / bound, f"{where} slot {s}"
        return got


def f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("stride", [1, 2])
def test_rowsum_and_rowmean(rows, stride):
    rng = np.random.default_rng(100 * rows + stride)
    x = f32(rng, max(rows, 1) * stride, scale=30.0)
    group = rng.integers(-1, 5, max(rows, 1)).astype(np.int32)                # -1 and 4: out of range for n_groups = 4, left out
    group[group == 2] = 3                                                     # group 2 stays empty
    t = Table()
    assert t.call([dict(kind=R.ROWSUM, slot=0, a=x, rows=rows, stride=stride),
                   dict(kind=R.ROWMEAN, slot=1, a=x, rows=rows, stride=stride),
                   dict(kind=R.ROWSUM, slot=2, a=x, rows=rows, stride=stride, n_groups=4, group=group),
                   dict(kind=R.ROWMEAN, slot=6, a=x, rows=rows, stride=stride, n_groups=4, group=group)]) == 0
    got = t.check(f"rows {rows} stride {stride}")
    assert got[0, 1] == rows and got[1, 1] == (1 if rows else 0)
    assert got[4, 1] == 0 and got[8, 1] == 0 and got[4, 0] == 0                                       # the empty group: untouched
    if rows == 0:
        assert not t.t.cpu().any()                                                                    # rows == 0 writes nothing


@pytest.mark.parametrize("rows", ROWS)
def test_match(rows):
    rng = np.random.default_rng(7 + rows)
    n = max(rows, 1)
    a, b = rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)
    b[rng.random(n) < 0.3] = -100
    group = rng.integers(0, 2, n).astype(np.int32)
    t = Table()
    assert t.call([dict(kind=R.MATCH, slot=0, a=a, b=b, rows=rows),
                   dict(kind=R.MATCH, slot=1, a=a, b=b, rows=rows, flags=R.INVERT),                   # all rows, -100 is a value like any
                   dict(kind=R.MATCH, slot=2, a=a, b=b, rows=rows, n_groups=2, group=group),
                   dict(kind=R.MATCH, slot=4, a=a, b=b, rows=rows, ignore_index=1),
                   dict(kind=R.MATCH, slot=5, a=a, b=b, rows=rows, n_groups=1, group=group)]) == 0    # n_groups = 1: group 1's rows left out
    got = t.check(f"match rows {rows}")
    assert got[1, 1] == rows and got[0, 1] == int((b[:rows] != -100).sum())


# every column count at 1 / 5 / 257 rows, and every row count (the wave-per-row loop: 0, one wave short of a round of four, whole rounds,
# one over, many rounds) at 3 and 65 columns - one lane pass and two
ARGMAX_SHAPES = [(r, c) for c in NCOLS for r in (1, 5, 257)] + [(r, c) for r in ROWS for c in (3, 65) if (r, c) not in ((1, 3), (1, 65), (257, 3), (257, 65))]


@pytest.mark.parametrize("rows,ncols", ARGMAX_SHAPES)
def test_argmax_match(rows, ncols):
    rng = np.random.default_rng(1000 * ncols + rows)
    pitch = ncols + 1 + ncols % 3
    if rows == 0:
        t = Table()
        t.t.copy_(torch.arange(2 * N_SLOTS, dtype=torch.float64).view(N_SLOTS, 2) * 0.1)
        t.ref.t[:] = t.t.cpu().numpy()
        before = t.buf.clone()
        z0, l0 = f32(rng, 1, pitch), np.zeros(1, np.int32)
        assert t.call([dict(kind=R.ARGMAX_MATCH, slot=0, a=z0, b=l0, rows=0, ncols=ncols),
                       dict(kind=R.ARGMAX_MATCH, slot=1, a=z0, b=l0, rows=0, ncols=ncols, flags=R.INVERT),
                       dict(kind=R.ARGMAX_MATCH, slot=2, a=z0, b=l0, rows=0, ncols=ncols, n_groups=4, group=l0)]) == 0
        torch.cuda.synchronize()
        assert torch.equal(t.buf, before)                                     # rows == 0: not a byte of the table is written
        return
    z = f32(rng, rows, pitch)
    z[:, ncols:] = 1e30                                                       # garbage in the pad columns: larger than any logit
    lab = rng.integers(0, ncols, rows).astype(np.int32)
    lab[::3] = R.argmax_first(z, ncols)[::3]                                  # a third of the rows hit for sure
    lab[1::5] = -100
    group = rng.integers(0, 4, rows).astype(np.int32)
    t = Table()
    assert t.call([dict(kind=R.ARGMAX_MATCH, slot=0, a=z, b=lab, rows=rows, ncols=ncols),
                   dict(kind=R.ARGMAX_MATCH, slot=1, a=z, b=lab, rows=rows, ncols=ncols, flags=R.INVERT),
                   dict(kind=R.ARGMAX_MATCH, slot=2, a=z, b=lab, rows=rows, ncols=ncols, n_groups=4, group=group)]) == 0
    got = t.check(f"argmax rows {rows} ncols {ncols}")
    assert got[0, 0] >= int((lab[::3] != -100).sum()) and got[1, 1] == rows


def test_argmax_ties_and_minus_inf_rows():
    """Exact ties: the FIRST maximum wins, with the tie at columns 0 / 63 / 64 / last; a row of -inf gives column 0."""
    ncols, pitch = 130, 136
    spots = [(0, 63), (63, 64), (64, 129), (0, 129), (63, 129), (5, 70)]
    z = f32(np.random.default_rng(3), len(spots) + 2, pitch)
    for r, (first, second) in enumerate(spots):
        z[r, first] = z[r, second] = 50.0
    z[-2, :] = -np.inf
    z[-1, :ncols] = -np.inf
    z[-1, 77] = -1e30                                                         # the only finite logit of the row
    want = np.array([s[0] for s in spots] + [0, 77], np.int32)
    assert (R.argmax_first(z, ncols) == want).all()
    t = Table()
    assert t.call([dict(kind=R.ARGMAX_MATCH, slot=0, a=z, b=want, rows=len(want), ncols=ncols),
                   dict(kind=R.ARGMAX_MATCH, slot=1, a=z, b=np.array([s[1] for s in spots] + [1, 76], np.int32), rows=len(want), ncols=ncols)]) == 0
    got = t.check("ties")
    assert tuple(got[0]) == (len(want), len(want)) and tuple(got[1]) == (0, len(want))


def test_all_labels_ignored_leave_the_table_bytes():
    t = Table()
    t.t.copy_(torch.arange(2 * N_SLOTS, dtype=torch.float64).view(N_SLOTS, 2) * 0.1)
    t.ref.t[:] = t.t.cpu().numpy()
    before = t.buf.clone()
    lab = np.full(70, -100, np.int32)
    assert t.call([dict(kind=R.ARGMAX_MATCH, slot=0, a=f32(np.random.default_rng(1), 70, 4), b=lab, rows=70, ncols=3),
                   dict(kind=R.MATCH, slot=1, a=np.zeros(70, np.int32), b=lab, rows=70),
                   dict(kind=R.PAIR, slot=2, a=np.array([0.0], np.float32), b=np.array([0.0], np.float32)),      # den == 0
                   dict(kind=R.SCALAR, slot=4, a=np.array([np.nan], np.float32), b=np.array([0.0], np.float32)), # a closed gate: the NaN stays out
                   dict(kind=R.ROWSUM, slot=3, a=np.ones(4, np.float32), rows=0)]) == 0
    torch.cuda.synchronize()
    assert torch.equal(t.buf, before)


def test_scalar_pair_eight_mixed_ops_and_three_accumulating_calls():
    t = Table()
    for step in range(3):                                                     # three calls accumulate into one table
        rng = np.random.default_rng(50 + step)
        z = f32(rng, 33, 8)
        x = f32(rng, 300, scale=5.0)
        ops = [dict(kind=R.SCALAR, slot=0, a=f32(rng, 1)),                                             # a device scalar
               dict(kind=R.SCALAR, slot=1, imm=0.1 * (step + 1), scale=2.5),                          # an immediate, scaled
               dict(kind=R.SCALAR, slot=2, a=f32(rng, 1), scale=-0.5, b=np.array([3.0], np.float32)),       # an open gate
               dict(kind=R.PAIR, slot=3, a=np.array([7.0 + step], np.float32), b=np.array([12.0], np.float32)),
               dict(kind=R.ROWSUM, slot=4, a=x, rows=150, stride=2),
               dict(kind=R.ROWMEAN, slot=5, a=x, rows=300, n_groups=2, group=rng.integers(0, 2, 300).astype(np.int32)),
               dict(kind=R.MATCH, slot=7, a=rng.integers(0, 2, 90).astype(np.int32), b=rng.integers(0, 2, 90).astype(np.int32), rows=90),
               dict(kind=R.ARGMAX_MATCH, slot=8, a=z, b=rng.integers(0, 8, 33).astype(np.int32), rows=33, ncols=8)]
        assert t.call(ops) == 0
        got = t.check(f"mixed call {step}")
    assert got[0, 1] == 3 and got[3, 1] == 36 and got[3, 0] == 24 and got[4, 1] == 450 and got[5, 1] == 3 and got[8, 1] == 99


def test_a_repeated_call_from_the_same_table_gives_the_same_bytes():
    rng = np.random.default_rng(9)
    x, z = f32(rng, 1000, scale=100.0), f32(rng, 257, 70)
    lab, group = rng.integers(0, 65, 257).astype(np.int32), rng.integers(0, 3, 1000).astype(np.int32)
    start = torch.rand(N_SLOTS, 2, dtype=torch.float64, device=DEV)
    out = []
    for _ in range(2):
        t = Table()
        t.t.copy_(start)
        assert t.call([dict(kind=R.ROWSUM, slot=0, a=x, rows=1000, n_groups=3, group=group), dict(kind=R.ROWMEAN, slot=3, a=x, rows=1000),
                       dict(kind=R.ARGMAX_MATCH, slot=4, a=z, b=lab, rows=257, ncols=65), dict(kind=R.SCALAR, slot=5, a=x[:1])]) == 0
        torch.cuda.synchronize()
        out.append(t.buf.clone())
    assert torch.equal(out[0], out[1])


def test_rejected_calls_leave_the_device_table_untouched():
    t = Table(8)
    t.t.copy_(torch.arange(16, dtype=torch.float64).view(8, 2))
    before = t.buf.clone()
    x = t.dev(np.ones(8, np.float32))
    i = t.dev(np.zeros(8, np.int32))
    ok = dict(kind=L.METRIC_SCALAR, slot=0, n_groups=1, scale=1.0)
    row = dict(kind=L.METRIC_ROWSUM, slot=0, n_groups=1, rows=4, stride=1, a=x.data_ptr())
    arg = dict(kind=L.METRIC_ARGMAX_MATCH, slot=0, n_groups=1, rows=2, ncols=2, pitch=4, a=x.data_ptr(), b=i.data_ptr())
    bad = [[], [ok] * 9, [dict(ok, slot=8)], [dict(ok, slot=-1)], [dict(row, slot=6, n_groups=3)], [dict(row, n_groups=0)], [dict(row, n_groups=5)],
           [dict(row, rows=-1)], [dict(row, a=None)], [dict(kind=L.METRIC_PAIR, slot=0, n_groups=1, a=x.data_ptr())],
           [dict(kind=L.METRIC_MATCH, slot=0, n_groups=1, rows=2, a=i.data_ptr())], [dict(arg, ncols=0)], [dict(arg, ncols=5)], [dict(arg, a=None)],
           [ok, dict(ok, slot=0)], [dict(row, n_groups=2), dict(ok, slot=1)]]
    for ops in bad:
        packed = L.MetricOps(n_ops=len(ops))
        for k, f in enumerate(ops[:L.METRIC_MAX_OPS]):
            packed.op[k] = L.MetricOp(**f)
        assert lib.rmcl_metrics_update(t.t.data_ptr(), 8, C.byref(packed), stream()) == -1, ops
    assert lib.rmcl_metrics_update(None, 8, C.byref(L.MetricOps(n_ops=1)), stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(t.buf, before)
