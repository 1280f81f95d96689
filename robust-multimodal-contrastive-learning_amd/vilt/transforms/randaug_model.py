"""numpy restatement of the fourteen RandAugment operations in PIL's own arithmetic - what resample.py is for the resize: the
specification csrc/randaug.hip is written from, pinned against PIL byte for byte on the CPU (tests/test_randaug_cpu.py).

``apply_op(img, code, p)``: img uint8 [h, w, 3], ``p`` the six doubles of ``randaug.plan_params``.  Three kinds of arithmetic occur:

  * integers: the histograms, Equalize's running sum, the luma (19595 R + 38470 G + 7471 B + 0x8000) >> 16, the 16.16 fixed-point
    source coordinates of Rotate / ShearX / ShearY;
  * doubles: AutoContrast's scale and offset, the Solarize threshold, SolarizeAdd's sum, the translations' source coordinate;
  * C float with SEPARATE multiply and add (numpy float32 never fuses): ``Image.blend`` of Color / Contrast / Brightness / Sharpness and
    the 3 x 3 SMOOTH filter behind Sharpness.  A fused multiply-add changes bytes (188 of the 65 536 (d, s) pairs at factor 1.36)."""
from __future__ import annotations

import numpy as np

from . import randaug as R

F32 = np.float32


def luma(img: np.ndarray) -> np.ndarray:
    """PIL's RGB -> L: uint8 [h, w]"""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def clip8(t: np.ndarray) -> np.ndarray:
    """float32 -> byte like PIL's clip: t <= 0 -> 0, t >= 255 -> 255, else truncate"""
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def blend(d: np.ndarray, s: np.ndarray, factor: float) -> np.ndarray:
    """``Image.blend(degenerate d, image s, factor)``: t = d + f * (s - d) in float32, unfused; truncated for 0 <= f <= 1, clipped otherwise"""
    f = F32(factor)
    di, si = d.astype(np.int32), s.astype(np.int32)
    t = di.astype(F32) + f * (si - di).astype(F32)
    if F32(0) <= f <= F32(1):
        return t.astype(np.int32).astype(np.uint8)
    return clip8(t)


def histograms(img: np.ndarray) -> np.ndarray:
    return np.stack([np.bincount(img[..., c].ravel(), minlength=256) for c in range(3)]).astype(np.int64)


def autocontrast_table(lo: int, hi: int) -> np.ndarray:
    """the 256-entry table of one channel whose first / last non-empty histogram bins are lo / hi"""
    i = np.arange(256)
    if hi <= lo:
        return i.astype(np.uint8)
    scale = np.float64(255.0) / np.float64(hi - lo)
    off = -np.float64(lo) * scale
    return np.clip((i.astype(np.float64) * scale + off).astype(np.int64), 0, 255).astype(np.uint8)      # (astype truncates toward zero, like int())


def equalize_table(h: np.ndarray) -> np.ndarray:
    nz = h[h > 0]
    i = np.arange(256)
    if nz.size <= 1:
        return i.astype(np.uint8)
    step = int(nz.sum() - nz[-1]) // 255
    if step == 0:
        return i.astype(np.uint8)
    n = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(n // step, 255).astype(np.uint8)


def mean_luma(img: np.ndarray) -> int:
    """int(ImageStat mean of L + 0.5) as (2 sum + N) // (2 N): the mean is a multiple of 1 / N, so it never comes within rounding
    distance of a half without being one"""
    n = img.shape[0] * img.shape[1]
    return int((2 * int(luma(img).astype(np.int64).sum()) + n) // (2 * n))


def lookup_tables(img: np.ndarray, code: int, p) -> np.ndarray:
    """uint8 [3, 256]: the table every lookup-class op (codes 0, 1, 3, 4, 5, 7, 8) applies per channel"""
    i = np.arange(256)
    if code == R.AUTOCONTRAST:
        out = []
        for h in histograms(img):
            nzb = np.nonzero(h)[0]
            out.append(autocontrast_table(int(nzb[0]), int(nzb[-1])))
        return np.stack(out)
    if code == R.EQUALIZE:
        return np.stack([equalize_table(h) for h in histograms(img)])
    if code == R.POSTERIZE:
        t = (i & ~(2 ** (8 - int(p[0])) - 1)).astype(np.uint8)
    elif code == R.SOLARIZE:
        t = np.where(i < np.float64(p[0]), i, 255 - i).astype(np.uint8)
    elif code == R.SOLARIZE_ADD:
        u = np.clip(i.astype(np.float64) + np.float64(p[0]), 0, 255).astype(np.uint8).astype(np.int64)
        t = np.where(u < 128, u, 255 - u).astype(np.uint8)
    elif code == R.CONTRAST:
        t = blend(np.full(256, mean_luma(img), np.uint8), i.astype(np.uint8), p[0])
    elif code == R.BRIGHTNESS:
        t = blend(np.zeros(256, np.uint8), i.astype(np.uint8), p[0])
    else:
        raise ValueError(f"op {code} is not a lookup op")
    return np.stack([t, t, t])


def fix16(v) -> int:
    """PIL's FIX: floor(v * 65536 + 0.5)"""
    return int(np.floor(np.float64(v) * 65536.0 + 0.5))


def gather_fixed(img: np.ndarray, a) -> np.ndarray:
    """NEAREST affine transform on PIL's 16.16 fixed-point path (Rotate, ShearX, ShearY)"""
    h, w, _ = img.shape
    a0, a1, a3, a4 = fix16(a[0]), fix16(a[1]), fix16(a[3]), fix16(a[4])
    a2 = fix16(a[2] + a[0] * 0.5 + a[1] * 0.5)
    a5 = fix16(a[5] + a[3] * 0.5 + a[4] * 0.5)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xin, yin = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def _scale_axis(start: float, n: int) -> np.ndarray:
    """source index per output index on PIL's scale path with unit step: the coordinate starts at start + 0.5 and grows by repeated
    addition of 1.0; negative -> -1 (outside), else truncated"""
    xo, out = np.float64(start) + np.float64(0.5), np.empty(n, np.int64)
    for i in range(n):
        out[i] = -1 if xo < 0 else int(xo)
        xo = xo + np.float64(1.0)
    return out


def gather_translate(img: np.ndarray, a) -> np.ndarray:
    h, w, _ = img.shape
    xin, yin = _scale_axis(a[2], w), _scale_axis(a[5], h)
    okx, oky = (xin >= 0) & (xin < w), (yin >= 0) & (yin < h)
    out = np.zeros_like(img)
    ys, xs = np.nonzero(oky)[0], np.nonzero(okx)[0]
    if ys.size and xs.size:
        out[np.ix_(ys, xs)] = img[np.ix_(yin[ys], xin[xs])]
    return out


def smooth(img: np.ndarray) -> np.ndarray:
    """ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13 in float32, rows y+1, y, y-1 in that order, each row (p0 k0 + p1 k1) + p2 k2 added to
    a sum that starts at 0.5; the one-pixel border is the source's; an image with a side below 3 comes back unchanged"""
    h, w, _ = img.shape
    out = img.copy()
    if h < 3 or w < 3:
        return out
    k1, k5 = F32(1) / F32(13), F32(5) / F32(13)
    f = img.astype(F32)
    ss = np.full((h - 2, w - 2, 3), F32(0.5), F32)
    for dy, kc in ((1, k1), (0, k5), (-1, k1)):
        rows = f[1 + dy: h - 1 + dy]
        ss = ss + ((rows[:, 0: w - 2] * k1 + rows[:, 1: w - 1] * kc) + rows[:, 2: w] * k1)
    out[1: h - 1, 1: w - 1] = clip8(ss)
    return out


def apply_op(img: np.ndarray, code: int, p) -> np.ndarray:
    code = int(code)
    if code in (R.AUTOCONTRAST, R.EQUALIZE, R.POSTERIZE, R.SOLARIZE, R.SOLARIZE_ADD, R.CONTRAST, R.BRIGHTNESS):
        t = lookup_tables(img, code, p)
        return np.stack([t[c][img[..., c]] for c in range(3)], axis=-1)
    if code == R.COLOR:
        return blend(np.repeat(luma(img)[..., None], 3, axis=2), img, p[0])
    if code == R.SHARPNESS:
        return blend(smooth(img), img, p[0])
    if code in (R.ROTATE, R.SHEAR_X, R.SHEAR_Y):
        return gather_fixed(img, p)
    if code in (R.TRANSLATE_X, R.TRANSLATE_Y):
        return gather_translate(img, p)
    raise ValueError(f"unknown RandAugment op code {code}")


def apply_plan(img: np.ndarray, plan) -> np.ndarray:
    h, w, _ = img.shape
    ops, params = R.plan_params(plan, w, h)
    for code, p in zip(ops, params):
        img = apply_op(img, code, p)
    return img
