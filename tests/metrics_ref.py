"""A float64 / integer numpy statement of the six op kinds of rmcl_metrics_update (include/rmcl.h), the reference of
tests/test_metrics_kernels_gpu.py, tests/test_epoch_metrics_cpu.py and tests/test_epoch_metrics_gpu.py.

Counts are integers; every sum is math.fsum of the exact double values of the fp32 addends, rounded once.  Next to the table the model
keeps, per slot, the sum of |addend| and the number of addends so far: a kernel that adds the same addends in double in ANY order stays
within ``addends * 2^-53 * sum|addend|`` of it (the rule of tests/test_guarded_step_kernels_gpu.py)."""
import math

import numpy as np

SCALAR, PAIR, ROWSUM, ROWMEAN, MATCH, ARGMAX_MATCH = range(6)
INVERT = 1


class RefTable:
    def __init__(self, n_slots):
        self.t = np.zeros((n_slots, 2), np.float64)
        self.abs = np.zeros(n_slots, np.float64)          # sum of |addend| into the slot's sum
        self.n = np.zeros(n_slots, np.int64)              # addends into the slot's sum (a row counts as one)

    def _add(self, slot, total, count, abs_total, n):
        self.t[slot, 0] += total
        self.t[slot, 1] += count
        self.abs[slot] += abs_total
        self.n[slot] += n

    def bound(self, slot):
        return float(self.n[slot]) * 2.0 ** -53 * float(self.abs[slot])

    def value(self, slot):
        s, c = self.t[slot]
        return s / c if c else None


def argmax_first(z, ncols=None):
    """index of the first maximum of every row over columns 0 .. ncols - 1 (numpy's argmax returns the first occurrence)"""
    z = np.asarray(z)
    return np.argmax(z[:, :ncols] if ncols is not None else z, axis=1).astype(np.int64)


def _groups(rows, n_groups, group):
    g = np.zeros(rows, np.int64) if group is None else np.asarray(group)[:rows].astype(np.int64)
    return [np.nonzero(g == j)[0] for j in range(n_groups)]


def apply(tab: RefTable, kind, slot, *, a=None, b=None, imm=0.0, scale=1.0, rows=0, stride=1, ncols=None, n_groups=1, group=None,
          ignore_index=-100, flags=0):
    """One op.  a / b: numpy arrays (fp32 values or int32 indices, flat; ARGMAX_MATCH: a = [rows, pitch])."""
    if kind == SCALAR:
        if b is not None and float(np.asarray(b).reshape(-1)[0]) == 0:        # the gate: nothing is added
            return
        x = np.float32(imm) if a is None else np.float32(np.asarray(a).reshape(-1)[0])
        v = float(np.float32(scale)) * float(x)               # (exact in double: two fp32 factors)
        tab._add(slot, v, 1, abs(v), 1)
    elif kind == PAIR:
        num, den = float(np.asarray(a).reshape(-1)[0]), float(np.asarray(b).reshape(-1)[0])
        if den != 0:
            tab._add(slot, num, den, abs(num), 1)
    elif kind in (ROWSUM, ROWMEAN):
        x = np.asarray(a, np.float32).reshape(-1)
        for j, idx in enumerate(_groups(rows, n_groups, group)):
            if len(idx) == 0:
                continue
            v = [float(x[r * stride]) for r in idx]
            if kind == ROWSUM:
                tab._add(slot + j, math.fsum(v), len(idx), math.fsum(map(abs, v)), len(v))
            else:
                tab._add(slot + j, math.fsum(v) / len(v), 1, math.fsum(map(abs, v)) / len(v), len(v) + 1)      # (+ 1: the division)
    elif kind in (MATCH, ARGMAX_MATCH):
        pred = argmax_first(np.asarray(a)[:rows], ncols) if kind == ARGMAX_MATCH else np.asarray(a).reshape(-1)[:rows].astype(np.int64)
        lab = np.asarray(b).reshape(-1)[:rows].astype(np.int64)
        for j, idx in enumerate(_groups(rows, n_groups, group)):
            if flags & INVERT:
                use, hit = idx, int((pred[idx] != lab[idx]).sum())
            else:
                use = idx[lab[idx] != ignore_index]
                hit = int((pred[use] == lab[use]).sum())
            if len(use):
                tab._add(slot + j, float(hit), len(use), float(hit), 1)
    else:
        raise ValueError(kind)
