"""RandAugment of the ``pixelbert_randaug`` transform (behaviour of the reference's vilt/transforms/randaug.py, inserted in front of
MinMaxResize by transforms/pixelbert.py:20-30), host side: PIL does the pixels.

The reference draws ``n`` operations with ONE ``random.choices(k=n)`` and then, inside every operation that has a sign (Rotate, the two
shears, the two translations), one ``random.random()``; no other operation consumes randomness.  So the whole PLAN - (op code, signed
value) per stage - can be drawn before a pixel is touched and still leave the ``random`` stream where the reference leaves it:
``draw_plan`` does that, ``apply_plan_pil`` executes a plan with PIL, ``plan_params`` encodes it for the device (rmcl_randaug_u8,
include/rmcl.h; the arithmetic is restated in randaug_model.py).  The op code is the position in the reference's live ``augment_list()``.

SolarizeAdd: the reference widens the pixels with ``np.array(img).astype(np.int)``, an alias numpy removed (AttributeError on numpy
>= 1.24); its arithmetic is reproduced with ``int``."""
from __future__ import annotations

import math
import random

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

# (code, name, min, max, draws a sign)
OPS = (
    (0, "AutoContrast", 0, 1, False),
    (1, "Equalize", 0, 1, False),
    (2, "Rotate", 0, 30, True),
    (3, "Posterize", 0, 4, False),
    (4, "Solarize", 0, 256, False),
    (5, "SolarizeAdd", 0, 110, False),
    (6, "Color", 0.1, 1.9, False),
    (7, "Contrast", 0.1, 1.9, False),
    (8, "Brightness", 0.1, 1.9, False),
    (9, "Sharpness", 0.1, 1.9, False),
    (10, "ShearX", 0.0, 0.3, True),
    (11, "ShearY", 0.0, 0.3, True),
    (12, "TranslateXabs", 0.0, 100, True),
    (13, "TranslateYabs", 0.0, 100, True),
)
AUTOCONTRAST, EQUALIZE, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y = range(14)
MAX_OPS = 8                      # include/rmcl.h RMCL_RA_MAX_OPS
FIXED_POINT_SIDE = 16384         # PIL leaves its 16.16 fixed-point path when a transformed corner reaches 32768


def magnitude(code: int, m) -> float:
    """the unsigned value of op `code` at magnitude m, in the reference's arithmetic"""
    _, _, lo, hi, _ = OPS[code]
    return (float(m) / 30) * float(hi - lo) + lo


def draw_plan(n: int, m, rng=random) -> list:
    """[(op code, signed value)] * n.  Consumes `rng` like the reference's ``RandAugment.__call__``: one ``choices(k=n)``, then one
    ``random()`` per operation that has a sign, in the order of the operations."""
    plan = []
    for code in rng.choices(range(len(OPS)), k=n):
        v = magnitude(code, m)
        if OPS[code][4] and rng.random() > 0.5:
            v = -v
        plan.append((int(code), v))
    return plan


def affine_coeffs(code: int, v: float, w: int, h: int) -> tuple:
    """the six coefficients (a, b, c, d, e, f) PIL's affine transform runs with: output (x, y) reads source (a x + b y + c, d x + e y + f).
    Rotate's are computed like ``Image.rotate`` computes them (Python doubles, rounded to 15 places, about the centre (w/2, h/2))."""
    if code == ROTATE:
        angle = v % 360.0
        if angle in (0, 90, 180, 270):
            raise ValueError(f"Rotate by {v}: multiples of 90 degrees take PIL's transpose paths, not the affine one")
        r = -math.radians(angle)
        mt = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
        cx, cy = w / 2, h / 2
        mt[2] = mt[0] * -cx + mt[1] * -cy + mt[2]
        mt[5] = mt[3] * -cx + mt[4] * -cy + mt[5]
        mt[2] += cx
        mt[5] += cy
        return tuple(mt)
    return {SHEAR_X: (1, v, 0, 0, 1, 0), SHEAR_Y: (1, 0, 0, v, 1, 0), TRANSLATE_X: (1, 0, v, 0, 1, 0), TRANSLATE_Y: (1, 0, 0, 0, 1, v)}[code]


def _solarize_add(img: Image.Image, addition, threshold=128) -> Image.Image:
    px = np.array(img).astype(int) + addition
    return ImageOps.solarize(Image.fromarray(np.clip(px, 0, 255).astype(np.uint8)), threshold)


def apply_op_pil(img: Image.Image, code: int, v: float) -> Image.Image:
    if code == AUTOCONTRAST:
        return ImageOps.autocontrast(img)
    if code == EQUALIZE:
        return ImageOps.equalize(img)
    if code == ROTATE:
        return img.rotate(v)
    if code == POSTERIZE:
        return ImageOps.posterize(img, max(1, int(v)))
    if code == SOLARIZE:
        return ImageOps.solarize(img, v)
    if code == SOLARIZE_ADD:
        return _solarize_add(img, v)
    if code in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        enhancer = {COLOR: ImageEnhance.Color, CONTRAST: ImageEnhance.Contrast, BRIGHTNESS: ImageEnhance.Brightness, SHARPNESS: ImageEnhance.Sharpness}[code]
        return enhancer(img).enhance(v)
    if code in (SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y):
        return img.transform(img.size, Image.AFFINE, affine_coeffs(code, v, *img.size))
    raise ValueError(f"unknown RandAugment op code {code}")


def apply_plan_pil(img: Image.Image, plan) -> Image.Image:
    for code, v in plan:
        img = apply_op_pil(img, int(code), float(v))
    return img


def apply_params_pil(img: Image.Image, ops, params) -> Image.Image:
    """a plan in the device encoding of ``plan_params`` executed with PIL: the affine ops hand their six coefficients to ``Image.transform``
    (the call ``Image.rotate`` ends in), the others read their value back from params[0]"""
    for code, p in zip(ops, params):
        code = int(code)
        if code in (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y):
            img = img.transform(img.size, Image.AFFINE, tuple(float(c) for c in p))
        else:
            img = apply_op_pil(img, code, float(p[0]))
    return img


class RandAugment:
    """callable(PIL image) -> PIL image: `n` operations at magnitude `m` out of 0..30 (the reference builds RandAugment(2, 9))"""

    def __init__(self, n: int, m):
        self.n, self.m = n, m

    def __call__(self, img: Image.Image) -> Image.Image:
        return apply_plan_pil(img, draw_plan(self.n, self.m))


def plan_params(plan, w: int, h: int):
    """(ops int32 [n], params float64 [n, 6]): the plan as rmcl_randaug_u8 takes it, for an image of w x h pixels - the six affine
    coefficients for Rotate, the shears and the translations; for the others params[0] = factor / threshold / bits / addition.  Raises
    for what the device arithmetic does not cover (the host applies such a plan: ``apply_plan_pil``)."""
    n = len(plan)
    if not 1 <= n <= MAX_OPS:
        raise ValueError(f"a plan holds 1..{MAX_OPS} operations (got {n})")
    ops, params = np.zeros(n, np.int32), np.zeros((n, 6), np.float64)
    for i, (code, v) in enumerate(plan):
        code, v = int(code), float(v)
        if not 0 <= code < len(OPS):
            raise ValueError(f"unknown RandAugment op code {code}")
        ops[i] = code
        if code in (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y):
            if max(w, h) > FIXED_POINT_SIDE:
                raise ValueError(f"{OPS[code][1]} on {w} x {h}: sides above {FIXED_POINT_SIDE} leave PIL's fixed-point path")
            params[i] = affine_coeffs(code, v, w, h)
            if code in (SHEAR_X, SHEAR_Y) and v == 0:
                raise ValueError("a shear of 0 takes PIL's scale path, not the fixed-point one")
            if code in (TRANSLATE_X, TRANSLATE_Y):
                # PIL steps the source coordinate by repeated addition of 1.0; the kernel forms start + x.  Both are exact unless the
                # start lies within rounding distance of an integer without being one
                frac = math.fmod(abs(v + 0.5), 1.0)
                if 0 < min(frac, 1 - frac) < 1e-9:
                    raise ValueError(f"translation by {v}: start coordinate too close to an integer for the device's direct form")
        elif code == POSTERIZE:
            params[i, 0] = max(1, int(v))
        else:
            params[i, 0] = v
    return ops, params
