"""A float64 / integer numpy statement of the contract of rmcl_rows_topk (include/rmcl.h), the reference of tests/test_topk_kernels_gpu.py
and tests/test_predict_gpu.py, with the rounding model its ``prob`` / ``lse`` allowance comes from (checked on the CPU in
tests/test_topk_ref_cpu.py).

Contract.  Per row of x [R, C]: the k first maxima in descending order - larger value first, equal values to the smaller column, -inf an
ordinary value that sorts last, NaN never selected; slots a row cannot fill hold idx -1, val -inf, prob 0.  val is the input element itself.
mode "softmax": prob = exp(val - lse), lse the log-sum-exp of the row's selectable (non-NaN) columns; a row without a finite column has
lse -inf and a selected -inf column has prob 0.  mode "sigmoid": prob = 1 / (1 + exp(-val)).

Rounding model (u = 2^-24, the fp32 unit round-off; expf / logf of the device library are taken at <= 2 ulp = 4u).  The kernel keeps a
running maximum m and s = sum exp(x - m) per thread over at most ceil(C / 1024) * 4 + 2 columns, then merges the 256 pairs in 6 butterfly
steps and 3 wave steps.  One step - adding a column, or merging two pairs - forms one difference d = x - m with |d| <= `spread` (the
largest minus the smallest finite entry of the row; relative error u in d, so |d| u in the exponent), one exp (4u), and at most one
multiplication and one addition (2u) on non-negative terms: a relative error of at most (spread + 6) u per step on the part of the sum it
touches.  With `steps` = ceil(C / 1024) * 4 + 2 + 9 sequential steps on the longest path, s carries at most steps * (spread + 6) u
(first order; the factor 1.01 covers the second).  lse = m + log(s) adds 4u |log s| for the log and u |lse| for the addition:
    lse_allow  = 1.01 * steps * (spread + 6) u + (4 |log s| + |lse|) u
prob = exp(val - lse): the difference is rounded (u |val - lse|), carries the lse error, and the exp adds 4u:
    prob_allow = prob * (lse_allow + (|val - lse| + 4) u) * 1.01 + 2^-126
sigmoid: exp (4u), one addition (u), one division (u):  prob * 6u * 1.01 + 2^-126.  The absolute term 2^-126 is the smallest normal fp32
number: a result below it may be flushed to zero (and where exp(-val) overflows fp32, val < -88.7, the kernel gives 0 for a value below
2^-127)."""
import math

import numpy as np

U = 2.0 ** -24
MODES = ("raw", "softmax", "sigmoid")


def order(row):
    """columns of one row in selection order: value descending, ties by column ascending, NaN columns left out"""
    row = np.asarray(row, dtype=np.float64)
    cols = np.flatnonzero(~np.isnan(row))
    return cols[np.lexsort((cols, -row[cols]))]               # (last key is the primary one; -(-inf) = +inf sorts last)


def lse_row(row):
    row = np.asarray(row, dtype=np.float64)
    fin = row[np.isfinite(row)]
    if fin.size == 0:
        return -np.inf
    m = fin.max()
    return float(m + np.log(np.exp(fin - m).sum()))


def rows_topk(x, k, mode="raw"):
    """(idx [R, k] int32, val [R, k] float32, prob [R, k] float64 or None, lse [R] float64 or None) of a float32 array x [R, C]"""
    assert mode in MODES
    x = np.asarray(x, dtype=np.float32)
    R, C = x.shape
    assert 1 <= k <= C
    idx = np.full((R, k), -1, dtype=np.int32)
    val = np.full((R, k), -np.inf, dtype=np.float32)
    prob = None if mode == "raw" else np.zeros((R, k))
    lse = np.array([lse_row(x[r]) for r in range(R)]) if mode == "softmax" else None
    for r in range(R):
        o = order(x[r])[:k]
        idx[r, : o.size] = o
        val[r, : o.size] = x[r, o]
        v = x[r, o].astype(np.float64)
        if mode == "softmax":
            with np.errstate(invalid="ignore"):
                prob[r, : o.size] = np.where(np.isneginf(v), 0.0, np.exp(v - lse[r]))
        elif mode == "sigmoid":
            with np.errstate(over="ignore"):
                prob[r, : o.size] = 1.0 / (1.0 + np.exp(-v))
    return idx, val, prob, lse


def steps(C):
    """sequential (add or merge) steps on the longest path of the kernel's log-sum-exp: a thread's columns, 6 butterfly + 3 wave merges"""
    return (C + 1023) // 1024 * 4 + 2 + 9


def lse_allowance(row):
    """|kernel lse - float64 lse| allowed for one row (0 where the row has no finite column: the kernel then writes -inf exactly)"""
    row = np.asarray(row, dtype=np.float64)
    fin = row[np.isfinite(row)]
    if fin.size == 0:
        return 0.0
    spread = float(fin.max() - fin.min())
    lse = lse_row(row)
    log_s = lse - float(fin.max())
    return 1.01 * steps(row.size) * (spread + 6.0) * U + (4.0 * abs(log_s) + abs(lse)) * U


def prob_allowance(row, val, prob, mode):
    """|kernel prob - float64 prob| allowed per selected entry of one row (val, prob: the float64 model's [k])"""
    val, prob = np.asarray(val, dtype=np.float64), np.asarray(prob, dtype=np.float64)
    if mode == "sigmoid":
        return prob * 6.0 * U * 1.01 + 2.0 ** -126
    lse = lse_row(row)
    d = np.where(np.isfinite(val), np.abs(val - lse), 0.0) if math.isfinite(lse) else np.zeros_like(val)
    return prob * (lse_allowance(row) + (d + 4.0) * U) * 1.01 + 2.0 ** -126


def kernel_lse_f32(row):
    """The kernel's summation order in numpy float32 (csrc/topk.hip): the row cut at its first 16-byte boundary (taken as column 0 here, as
    for an aligned row), thread t owns the float4 groups t, t + 256, ... and tail column j for t = 8 + j; per thread a running maximum
    and sum over its columns in ascending order, then the butterfly over each wave's 64 lanes and the four waves in order."""
    f = np.float32
    row = np.asarray(row, dtype=f)
    C = row.size
    G = C // 4

    def add(x, m, s):
        if not x > f(-np.inf):
            return m, s
        if x > m:
            return x, f(f(s * np.exp(f(m - x), dtype=f)) + f(1.0))
        return m, f(s + np.exp(f(x - m), dtype=f))

    def merge(m1, s1, m2, s2):
        M = max(m1, m2)
        if not M > f(-np.inf):
            return M, s1
        return M, f(f(s1 * np.exp(f(m1 - M), dtype=f)) + f(s2 * np.exp(f(m2 - M), dtype=f)))

    ms = []
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(256):
            m, s = f(-np.inf), f(0.0)
            for g in range(t, G, 256):
                for x in row[4 * g: 4 * g + 4]:
                    m, s = add(x, m, s)
            c = 4 * G + t - 8
            if t >= 8 and c < C:
                m, s = add(row[c], m, s)
            ms.append((m, s))
        waves = []
        for w in range(4):
            lanes = ms[64 * w: 64 * w + 64]
            for o in (32, 16, 8, 4, 2, 1):
                lanes = [merge(*lanes[i], *lanes[i ^ o]) for i in range(64)]
            waves.append(lanes[0])
        m, s = waves[0]
        for w in range(1, 4):
            m, s = merge(m, s, *waves[w])
        return float(f(m + np.log(s, dtype=f))) if s > 0 else -np.inf
