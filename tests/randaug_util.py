"""Shared by the RandAugment tests and tools/gen_golden_randaug.py: the formula-generated source images of tests/golden/randaug.npz, the
test images and sizes of the per-op comparisons against PIL, and the single-op cases."""
import numpy as np

from rmcl_amd.vilt.transforms import randaug as R

FIXTURE_SIZES = ((60, 50), (97, 131))            # (w, h) of the two source images of the fixture
FIXTURE_SEED = 20240
SAMPLE_STRIDE = 53                               # the fixture keeps every 53rd byte of an output (and a digest of all of them)
SIZES = ((1, 1), (2, 5), (5, 2), (3, 3), (60, 50), (97, 131), (33, 200), (64, 256), (65, 257))     # (w, h)
MAGNITUDES = (9, 21, 30)


def source_image(w: int, h: int, seed: int) -> np.ndarray:
    """uint8 [h, w, 3] in integer arithmetic only (no libm, no generator whose stream could change): a triangle wave over 5x + 3y scaled into
    [40 + 10c, 190 + 10c] plus hashed noise in [-30, 30] - every channel's histogram starts above 0 and ends below 255."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(3, dtype=np.uint64), indexing="ij")
    m32 = np.uint64(0xFFFFFFFF)
    k = ((x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ (c * np.uint64(83492791)) ^ (np.uint64(seed) * np.uint64(2654435761))) & m32
    k = (k * np.uint64(2654435761)) & m32
    k ^= k >> np.uint64(15)
    noise = (k % np.uint64(61)).astype(np.int64) - 30
    tri = np.abs(((x * np.uint64(5) + y * np.uint64(3)) % np.uint64(512)).astype(np.int64) - 256)
    return np.clip(40 + 10 * c.astype(np.int64) + tri * 150 // 256 + noise, 0, 255).astype(np.uint8)


def fixture_images():
    return [source_image(w, h, FIXTURE_SEED + i) for i, (w, h) in enumerate(FIXTURE_SIZES)]


def strided(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).ravel()[::SAMPLE_STRIDE].copy()


def single_cases():
    """[(op code, m, signed value)]: every op alone at m = 9, 21, 30, the signed ops with both signs"""
    out = []
    for code, _, _, _, signed in R.OPS:
        for m in MAGNITUDES:
            v = R.magnitude(code, m)
            out.append((code, m, v))
            if signed:
                out.append((code, m, -v))
    return out


def noise_image(w: int, h: int, seed: int) -> np.ndarray:
    """uniform noise over the whole byte range"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_image(w: int, h: int, seed: int) -> np.ndarray:
    """gradients and edges plus noise, kept inside [24, 230]: histograms that end inside the byte range"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 70 * np.sin(xx / 17.0)[..., None] * np.cos(yy / 23.0)[..., None] + np.array([-12.0, 0.0, 9.0])
    return (base + rng.normal(0, 12, (h, w, 3))).clip(24, 230).astype(np.uint8)
