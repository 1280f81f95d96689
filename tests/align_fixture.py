"""CPU side of the alignment fixture tests/golden/align_L2.npz (test infrastructure): the seeded batches on the toy vocabulary, the
demo's masks, and the margins under which a recorded decision may be asked of an engine whose cost differs from the reference's.
tools/gen_golden_align.py runs the reference's own model, cost_matrix_cosine and ipot and the demo's heat arithmetic and records them;
tests/test_align_ref_cpu.py pins the record against the float64 model of tests/align_ref.py; tests/test_align_gpu.py asks the same of
``rmcl_amd.Predictor.align``.

Cases.  "square": one 128 x 128 image (4 x 4 patches, all kept) and a sentence of 18 tokens - the demo's masks leave 16 positions.
"ragged": a zero-padded pair of a 96 x 128 and a 64 x 96 image (a 3 x 4 grid; 12 and 6 kept patches, so the second sample has six
padding slots and six cells that stay 0) with sentences of 14 and 8 tokens (12 and 6 live positions).  As many live words as kept
patches on purpose: both marginals of the plan are uniform, so where the counts differ a word owns several whole patches whose plan
entries are EQUAL (each pinned at 1 / patches by its row sum) - the arg-max of such a map is decided by the last bit in the reference
itself, and no seed passes the margin condition below.  With equal counts the converged plan is close to a permutation and every map
has one owner; at 50 iterations it is still spread out and the bytes take intermediate values.

Margins.  After t iterations the plan behaves like exp(-t C / beta) rescaled, so a cost that is off by dC moves an entry by a relative
4 t dC / beta at most (one such term each from the numerator, delta and sigma, one for margin).  The generator assumes
dC <= DC_BUDGET = 2e-6 (16 ulp of a cost near 1: the fp32 engine's features are held to the reference's far closer than that, and the
test asserts the dC it measures against the budget before it relies on a margin), perturbs every grid by that relative amount in
6 + N_RANDOM sign patterns - all up, all down, the largest cell against the rest both ways, the second largest against the rest both
ways, and seeded random signs - and refuses a seed in which the set of non-zero heat cells or the arg-max cell of any recorded map changes under any of
them.  A byte is recorded as stable (byte_ok) where it is the same under every pattern and 255 * heat is exactly 0 or 255, or at least
BYTE_MARGIN from the next integer, in the float64 model."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import rmcl_oracle as O
from tests import align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "toy_vocab.txt")
FIXTURE = "align_L2.npz"
CASES = {"square": dict(B=1, sizes=[(128, 128)], lens=[18]), "ragged": dict(B=2, sizes=[(96, 128), (64, 96)], lens=[14, 8])}
WORD0, WORD1 = 1000, 1143
SEEDS = dict(weights=11, batch=40)
BETA = 0.1
ITERS = (50, 1000)
DC_BUDGET = 2e-6
BYTE_MARGIN = 1e-3
N_RANDOM = 32


def config():
    return O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=2)


def make_batch(cfg, case: str):
    c = CASES[case]
    seed = SEEDS["batch"] + list(CASES).index(case)
    batch = O.synthetic_batch(cfg, c["B"], seed, sizes=c["sizes"])
    g = torch.Generator().manual_seed(seed + 1)
    ids = torch.randint(WORD0, WORD1, batch["text_ids"].shape, generator=g)
    masks = torch.zeros_like(batch["text_masks"])
    for b, n in enumerate(c["lens"]):                      # [CLS] w ... w [SEP], then padding
        ids[b, 0], ids[b, n - 1], ids[b, n:], masks[b, :n] = 101, 102, 0, 1
    batch["text_ids"], batch["text_masks"] = ids, masks
    return batch


def demo_masks(text_masks, image_masks):
    """(txt_valid [B, Lt], img_valid [B, Li]) bool: demo.py:97-105 - [CLS], the last valid text token and the image cls slot dropped"""
    t, i = torch.as_tensor(text_masks).bool().clone(), torch.as_tensor(image_masks).bool().clone()
    for b, n in enumerate(t.sum(dim=1)):
        t[b, n - 1] = False
    t[:, 0] = False
    i[:, 0] = False
    return t, i


def relative_bound(t: int, dC: float) -> float:
    return 4.0 * t * dC / BETA


def patterns(g, seed):
    """sign patterns [K, H W] for one grid g [H, W]"""
    flat = np.asarray(g, dtype=np.float64).reshape(-1)
    n = flat.size
    order = np.argsort(-flat, kind="stable")
    pats = [np.ones(n), -np.ones(n)]
    for k in range(min(2, n)):
        s = -np.ones(n)
        s[order[k]] = 1.0
        pats += [s, -s]
    rng = np.random.RandomState(seed)
    pats += [rng.choice([-1.0, 1.0], size=n) for _ in range(N_RANDOM)]
    return np.stack(pats)


def stability(g, r, seed):
    """(stable, byte_ok [H, W]) of one non-flat grid under the relative perturbation r: stable = the non-zero set and the arg-max of the
    heat map are those of the unperturbed grid under every pattern"""
    g = np.asarray(g, dtype=np.float64)
    heat, flat = R.heat_one(g)
    assert not flat
    by = R.alpha_bytes(heat, *g.shape)
    ok = R.byte_margin(heat) >= BYTE_MARGIN
    stable = True
    for s in patterns(g, seed):
        h2, f2 = R.heat_one(g * (1.0 + r * s.reshape(g.shape)))
        if f2 or not np.array_equal(h2 > 0, heat > 0) or int(h2.argmax()) != int(heat.argmax()):
            stable = False
            continue
        ok &= R.alpha_bytes(h2, *g.shape) == by
    return stable, ok
