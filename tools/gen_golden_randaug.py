"""Generate tests/golden/randaug.npz by running the REFERENCE's own vilt/transforms/randaug.py (RandAugment(2, 9) and each of the fourteen
live operations alone) on two formula-generated source images (tests/randaug_util.py source_image).

TEST INFRASTRUCTURE ONLY: runs on the build machine only - it loads randaug.py out of the reference checkout (the directory given by
--reference or the environment variable RMCL_REFERENCE); no test reads the reference.  The reference's SolarizeAdd widens with
``np.array(img).astype(np.int)``, an alias numpy removed: ``np.int = int`` is set for this run only.

Recorded, per source image:
  * for 40 values of ``random.seed``: the op codes RandAugment(2, 9) chose (positions in the reference's ``augment_list()``), the SIGNED values
    the operations ran with, ``random.random()`` right after the call (the state the reference leaves the stream in), a digest of the output
    (tests/golden_util.digest) and every 53rd byte of it;
  * for each of the 14 ops alone at m = 9, 21, 30 (both signs for the ops that draw one): the signed value, the digest and the byte sample.
The reference's ops draw their sign from the module ``random`` they import; a proxy in its place logs every ``random()`` the run makes (the
seeded runs) or returns a fixed draw (the single-op records: 0.25 keeps the sign, 0.75 flips it).

Usage:  python tools/gen_golden_randaug.py [--reference DIR]      (writes tests/golden/randaug.npz, seconds)
"""
from __future__ import annotations

import argparse
import functools
import importlib.util
import os
import random
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rmcl_pkg  # noqa: F401,E402
from tests import golden_util  # noqa: E402
from tests import randaug_util as U  # noqa: E402

N_SEEDS = 40


class RandomProxy:
    """stands where the reference's ``random`` module stands: forwards to the real module and logs random(), or returns `fixed`"""

    def __init__(self, fixed=None):
        self.fixed, self.draws = fixed, []

    def choices(self, *a, **k):
        return random.choices(*a, **k)

    def random(self):
        v = random.random() if self.fixed is None else self.fixed
        self.draws.append(v)
        return v


def load_reference(ref_dir):
    path = os.path.join(ref_dir, "vilt", "transforms", "randaug.py")
    spec = importlib.util.spec_from_file_location("reference_randaug", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(out_img):
    a = np.asarray(out_img)
    return golden_util.digest(torch.from_numpy(a.copy())), U.strided(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("RMCL_REFERENCE", ""))
    args = ap.parse_args()
    if not os.path.isdir(args.reference):
        raise SystemExit("gen_golden_randaug.py: give the reference checkout with --reference DIR (or RMCL_REFERENCE)")
    had_int = hasattr(np, "int")
    if not had_int:
        np.int = int                                   # (this run only: the alias the reference's SolarizeAdd reads)
    try:
        ref = load_reference(args.reference)
        ops = ref.augment_list()
        names = [fn.__name__ for fn, _, _ in ops]
        out = {"op_names": np.array(names), "op_min": np.array([float(lo) for _, lo, _ in ops]), "op_max": np.array([float(hi) for _, _, hi in ops]),
               "img_sizes": np.array(U.FIXTURE_SIZES, np.int32), "img_seed": np.array(U.FIXTURE_SEED),
               "img_formula": np.array("tests/randaug_util.py source_image(w, h, img_seed + index)"), "sample_stride": np.array(U.SAMPLE_STRIDE),
               "draw_seeds": np.arange(N_SEEDS, dtype=np.int32)}
        images = U.fixture_images()
        out["img_digest"] = np.stack([golden_util.digest(torch.from_numpy(im)) for im in images])

        # ---- RandAugment(2, 9) under 40 seeds ----
        codes = np.zeros((len(images), N_SEEDS, 2), np.int32)
        values = np.zeros((len(images), N_SEEDS, 2), np.float64)
        nxt = np.zeros((len(images), N_SEEDS), np.float64)
        for k, im in enumerate(images):
            digs, samples = [], []
            for s in range(N_SEEDS):
                ra = ref.RandAugment(2, 9)
                seen = []

                def tap(i, fn, seen=seen):
                    @functools.wraps(fn)
                    def run(img, v):
                        before = len(ref.random.draws)
                        res = fn(img, v)
                        drawn = ref.random.draws[before:]
                        assert len(drawn) <= 1
                        seen.append((i, -v if drawn and drawn[0] > 0.5 else v))
                        return res
                    return run
                ra.augment_list = [(tap(i, fn), lo, hi) for i, (fn, lo, hi) in enumerate(ra.augment_list)]
                ref.random = RandomProxy()
                random.seed(s)
                res = ra(Image.fromarray(im))
                nxt[k, s] = random.random()
                assert len(seen) == 2 and res.size == (im.shape[1], im.shape[0])
                codes[k, s], values[k, s] = [c for c, _ in seen], [v for _, v in seen]
                d, smp = record(res)
                digs.append(d)
                samples.append(smp)
            out[f"draw_digest_{k}"], out[f"draw_sample_{k}"] = np.stack(digs), np.stack(samples)
        out["draw_codes"], out["draw_values"], out["draw_next_random"] = codes, values, nxt

        # ---- every op alone ----
        cases = U.single_cases()
        out["single_codes"] = np.array([c for c, _, _ in cases], np.int32)
        out["single_m"] = np.array([m for _, m, _ in cases], np.int32)
        out["single_values"] = np.array([v for _, _, v in cases], np.float64)
        for k, im in enumerate(images):
            digs, samples = [], []
            for code, m, v in cases:
                fn, lo, hi = ops[code]
                val = (float(m) / 30) * float(hi - lo) + lo                     # the reference's own expression (RandAugment.__call__)
                assert abs(v) == val, (code, m, v, val)
                ref.random = RandomProxy(fixed=0.75 if v < 0 else 0.25)
                d, smp = record(fn(Image.fromarray(im), val))
                digs.append(d)
                samples.append(smp)
            out[f"single_digest_{k}"], out[f"single_sample_{k}"] = np.stack(digs), np.stack(samples)
    finally:
        if not had_int:
            del np.int
    path = os.path.join(golden_util.GOLDEN, "randaug.npz")
    golden_util.save(path, out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {N_SEEDS} seeded draws and {len(cases)} single-op records per image; "
          f"ops drawn: {sorted(set(codes.ravel().tolist()))}")


if __name__ == "__main__":
    main()
