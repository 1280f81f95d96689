"""Numpy statements of the contracts of rmcl_ipot_plan_f32 and rmcl_align_heat (include/rmcl.h), the references of
tests/test_align_kernels_gpu.py and tests/test_align_gpu.py, checked on the CPU in tests/test_align_ref_cpu.py.

nearest_table    PIL's NEAREST source indices: xo = 0.5 * src / dst; idx[x] = min(int(xo), src - 1); xo += src / dst, accumulated in
                 double.  (The closed form floor((x + 0.5) * src / dst) is NOT PIL's: the accumulated centre drifts by a few ulp and lands
                 on the other side of an integer at some sizes, 12 x 19 -> 333 x 500 among them.)
scatter          grid[b, m, cell patch_index[b, i]] = T[b, 1 + i, m]; the image cls row is dropped; entries of patch_index outside
                 [0, H W) write nothing; every other cell is 0 (the demo's torch.zeros(H, W)).
heat_model       the demo's arithmetic (demo.py:141-143) in float64 over the whole grid: z = (g - mean) / std (unbiased), c = clip(z, 1, 3),
                 heat = (c - min c) / (max c - min c).  The demo's factor len(txt_emb) multiplies g, mean and std alike and cancels.
                 Deviation: where the demo divides by zero - a text position the masks drop, H W < 2, std == 0, max c == min c - heat is 0
                 and flat is 1; the demo produces NaN there.
alpha_bytes      np.uint8(float32(heat) * 255) - the demo forms the product in fp32 and np.uint8 truncates - enlarged by the two tables.
ipot_plan_f32    the summation order of csrc/align.hip in numpy float32 (no fused multiply-add): q = A * T; the row dot product with m
                 ascending; u = delta * q; per column and wave a balanced binary tree over the 64 lanes (wave_sum_dpp: lanes i and
                 i ^ 1, quads, mirrored halves of 8, of 16, rows 0 + 1 and 2 + 3, then the two halves; fp32 addition commutes, so only
                 the tree's shape matters) of (u of row n) + (u of row n + 256); the four waves as ((w0 + w1) + w2) + w3;
                 T = u * sigma.  expf and the division are the host's; the device's differ by an ulp or two.

Rounding model of heat (heat_allowance).  The kernel accumulates the mean, the sum of squared deviations and the extrema in fp64 from
the fp32 cells and rounds heat to fp32 once; with v = 2^-53 and n = H W terms:
    mean      relative error <= n v                      (n additions of non-negative terms, one division)
    d = g - mean   absolute error <= |mean| n v + |d| v
    std       relative error <= (n + 4) v + 2 |mean| n v sum|d| / sum d^2   (squares, n additions, a division, a square root)
    z = d / std    absolute error e_z <= (|mean| / std) n v + |z| (n + 6) v + |z| * (the second term of std), taken at |z| <= 3 after
              the clip (clip is 1-Lipschitz) and, generously, with the second term of std bounded through sum|d| <= sqrt(n sum d^2):
              e_z <= (1 + 6 sqrt(n / (n - 1))) (|mean| / std) n v + 3 (n + 6) v
    heat = (c - lo) / (hi - lo): numerator and denominator each carry 2 e_z, the quotient is at most 1:
              |heat error| <= 4 e_z / (hi - lo) + 4 v + 2^-24 heat     (the last term: the one rounding to fp32)
The float64 model itself carries errors of the same size; heat_allowance returns twice the bound."""
import numpy as np

V64 = 2.0 ** -53
U32 = 2.0 ** -24


def nearest_table(src: int, dst: int) -> np.ndarray:
    step = np.float64(src) / np.float64(dst)
    xo = np.float64(0.5) * step
    out = np.empty(dst, dtype=np.int64)
    for x in range(dst):
        out[x] = min(int(xo), src - 1)
        xo = xo + step
    return out


def nearest_table_closed_form(src: int, dst: int) -> np.ndarray:
    """what PIL does NOT do (kept for the test that shows the difference)"""
    return np.minimum(np.floor((np.arange(dst) + 0.5) * src / dst).astype(np.int64), src - 1)


def scatter(T, patch_index, H, W):
    """T [B, Li, Lt], patch_index [B, Li - 1] -> grid [B, Lt, H, W] of T's dtype"""
    T, patch_index = np.asarray(T), np.asarray(patch_index)
    B, Li, Lt = T.shape
    grid = np.zeros((B, Lt, H * W), dtype=T.dtype)
    for b in range(B):
        for i in range(Li - 1):
            c = int(patch_index[b, i])
            if 0 <= c < H * W:
                grid[b, :, c] = T[b, 1 + i, :]
    return grid.reshape(B, Lt, H, W)


def heat_one(g, valid=True):
    """(heat [H, W] float64, flat) of one grid"""
    g = np.asarray(g, dtype=np.float64)
    zero = np.zeros_like(g)
    if not valid or g.size < 2:
        return zero, 1
    mean = g.sum() / g.size
    sd = np.sqrt(((g - mean) ** 2).sum() / (g.size - 1))
    if not sd > 0:
        return zero, 1
    c = np.clip((g - mean) / sd, 1.0, 3.0)
    lo, hi = c.min(), c.max()
    if not hi > lo:
        return zero, 1
    return (c - lo) / (hi - lo), 0


def heat_model(grid, txt_valid):
    """grid [B, Lt, H, W], txt_valid [B, Lt] -> (heat float64 [B, Lt, H, W], flat int32 [B, Lt])"""
    grid = np.asarray(grid)
    B, Lt = grid.shape[:2]
    heat = np.zeros(grid.shape, dtype=np.float64)
    flat = np.zeros((B, Lt), dtype=np.int32)
    for b in range(B):
        for m in range(Lt):
            heat[b, m], flat[b, m] = heat_one(grid[b, m], bool(txt_valid[b, m]))
    return heat, flat


def heat_allowance(g):
    """the largest |kernel heat - model heat| the rounding model above allows on one non-flat grid (a scalar)"""
    g = np.asarray(g, dtype=np.float64)
    n = g.size
    mean = g.sum() / n
    sd = np.sqrt(((g - mean) ** 2).sum() / (n - 1))
    c = np.clip((g - mean) / sd, 1.0, 3.0)
    span = c.max() - c.min()
    e_z = (1 + 6 * np.sqrt(n / (n - 1.0))) * (abs(mean) / sd) * n * V64 + 3 * (n + 6) * V64
    return 2.0 * (4 * e_z / span + 4 * V64 + U32)


def alpha_bytes(heat, Hout, Wout):
    """heat [H, W] (any float type) -> uint8 [Hout, Wout]"""
    heat = np.asarray(heat)
    by = (heat.astype(np.float32) * np.float32(255.0)).astype(np.int32).astype(np.uint8)
    return by[nearest_table(heat.shape[0], Hout)][:, nearest_table(heat.shape[1], Wout)]


def byte_margin(heat64):
    """distance of 255 * heat from the nearest integer, per cell; cells at exactly 0 or 1 (bytes 0 and 255, values the arithmetic
    produces exactly: c - lo = 0 and (hi - lo) / (hi - lo) = 1) get +inf"""
    x = 255.0 * np.asarray(heat64, dtype=np.float64)
    d = np.abs(x - np.rint(x))
    d[(heat64 == 0.0) | (heat64 == 1.0)] = np.inf
    return d


def _tree64(x):
    """balanced binary tree over the last axis (64 lanes), float32"""
    while x.shape[-1] > 1:
        x = (x[..., 0::2] + x[..., 1::2]).astype(np.float32)
    return x[..., 0]


def ipot_plan_f32(cost, txt_valid, img_valid, beta, iters):
    """cost [B, Lt, ld >= Li] float32, masks [B, Lt] / [B, Li] -> T [B, Li, Lt] float32 in the kernel's summation order"""
    f = np.float32
    cost, tv, iv = np.asarray(cost, dtype=f), np.asarray(txt_valid) != 0, np.asarray(img_valid) != 0
    B, Lt, _ = cost.shape
    Li = iv.shape[1]
    rows = 256 if Li <= 256 else 512
    out = np.zeros((B, Li, Lt), dtype=f)
    for b in range(B):
        x_cnt, y_cnt = int(tv[b].sum()), int(iv[b].sum())
        if x_cnt == 0 or y_cnt == 0:
            continue
        x_len, y_len = f(x_cnt), f(y_cnt)
        ok = iv[b][:, None] & tv[b][None, :]                                  # [Li, Lt]
        A = np.zeros((rows, Lt), dtype=f)
        T = np.zeros((rows, Lt), dtype=f)
        A[:Li] = np.where(ok, np.exp((-cost[b, :, :Li].T / f(beta)).astype(f)).astype(f), f(0))
        T[:Li] = ok.astype(f)
        y_mask = np.full(rows, 1e4, dtype=f)
        y_mask[:Li][iv[b]] = 0
        x_mask = np.where(tv[b], f(0), f(1e4)).astype(f)
        sg = np.where(tv[b], f(1) / x_len, f(0)).astype(f)
        for _ in range(iters):
            q = (A * T).astype(f)
            s = np.zeros(rows, dtype=f)
            for m in range(Lt):
                s = (s + (q[:, m] * sg[m]).astype(f)).astype(f)
            delta = (f(1) / ((y_len * s).astype(f) + y_mask).astype(f)).astype(f)
            u = (delta[:, None] * q).astype(f)
            c = u[:256] if rows == 256 else (u[:256] + u[256:]).astype(f)     # per thread: row n + row n + 256
            w = _tree64(c.T.reshape(Lt, 4, 64))                               # [Lt, 4]: per column and wave
            p = (((w[:, 0] + w[:, 1]).astype(f) + w[:, 2]).astype(f) + w[:, 3]).astype(f)
            sg = (f(1) / ((x_len * p).astype(f) + x_mask).astype(f)).astype(f)
            T = (u * sg[None, :]).astype(f)
        out[b] = np.where(ok, T[:Li], f(0))
    return out
