"""Helpers shared by the golden-fixture tests (data only: the .npz files were written by
oracle/gen_golden.py from the reference's own arithmetic)."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 768 * 1024      # raw bytes above which save() cuts an array into side files (every fixture file stays under 1 MiB)


class Fixture(dict):
    """A fixture joined from <stem>.npz and its side files <stem>.partN.npz (the part of np.load's NpzFile the tests use)."""

    @property
    def files(self):
        return list(self.keys())


def save(path, out):
    """np.savez_compressed(path, **out), except that an array of more than PART_BYTES is cut along axis 0 into the side files
    <stem>.part1.npz, <stem>.part2.npz, ... that load() concatenates again in that order."""
    main, parts = {}, []
    for k, v in out.items():
        v = np.asarray(v)
        if v.nbytes <= PART_BYTES or v.ndim == 0 or v.shape[0] < 2:
            main[k] = v
            continue
        rows = max(1, PART_BYTES // (v.nbytes // v.shape[0]))
        for i, r0 in enumerate(range(0, v.shape[0], rows)):
            if i == len(parts):
                parts.append({})
            parts[i][k] = v[r0:r0 + rows]
    np.savez_compressed(path, **main)
    stem = path[:-len(".npz")]
    for f in glob.glob(glob.escape(stem) + ".part*.npz"):
        os.remove(f)
    for i, p in enumerate(parts):
        np.savez_compressed(f"{stem}.part{i + 1}.npz", **p)


def load(name):
    path = os.path.join(GOLDEN, name)
    stem = path[:-len(".npz")]
    n_parts = len(glob.glob(glob.escape(stem) + ".part*.npz"))
    if n_parts == 0:
        return np.load(path, allow_pickle=False)
    g = Fixture()
    for f in [path] + [f"{stem}.part{i + 1}.npz" for i in range(n_parts)]:
        with np.load(f, allow_pickle=False) as z:
            for k in z.files:
                g[k] = np.concatenate([g[k], z[k]]) if k in g else z[k]
    return g


def digest(t: torch.Tensor) -> np.ndarray:
    f = t.detach().double().flatten().cpu()
    head = torch.zeros(8, dtype=torch.float64)
    head[: min(8, f.numel())] = f[:8]
    return torch.cat([torch.stack([f.sum(), f.norm(), f.abs().max()]), head]).numpy()


def cfg_from_meta(O, meta, kind="moco"):
    if kind == "moco":
        B, seed_w, seed_b, ragged, L, Kq, K = [int(x) for x in meta]
        cfg = O.default_config(num_layers=L, num_negative=Kq, adv_steps_img=K, per_gpu_batchsize=B)
    else:
        B, seed_w, seed_b, ragged, L = [int(x) for x in meta]
        cfg = O.default_config(num_layers=L, per_gpu_batchsize=B)
    return cfg, B, seed_w, seed_b, bool(ragged)
