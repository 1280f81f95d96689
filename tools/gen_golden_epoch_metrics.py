"""tests/golden/epoch_metrics.json + epoch_metrics.npz: what the REFERENCE's own metric classes (vilt/gadgets/my_metrics.py), its
``set_metrics`` and its ``epoch_wrapup`` (vilt/modules/vilt_utils.py:13-313) create and log, recipe by recipe, for a train and a val epoch.

TEST INFRASTRUCTURE ONLY: runs on the build machine (needs the reference checkout that oracle/gen_golden.py imports).  The reference's
modules are loaded under the usual stand-ins (oracle/gen_golden.py) plus two: Lightning is not installed, so ``pytorch_lightning.metrics.
Metric`` is the minimal base below (``add_state`` / ``reset`` / ``__call__`` -> ``update``), and ``transformers.optimization.AdamW``, which
the installed transformers no longer has and the wrap-up never touches, is torch's.

A stub module records ``log``.  Each step feeds the metric attributes what the reference's objectives feed them (objectives.py:604-1223):
losses, logits and labels, soft targets, the dev / test subsets of a validation batch by ``table_name``.  One NLVR2 validation step has no
``test`` row, one MLM validation step has no labelled row: its cross-entropy is NaN, the reference's epoch loss with it; this package
adds a batch's MLM / MPP loss only when the batch has a labelled row (``gate`` of the call holds the count).  The reference's
nlvr2_attacked train branch creates ``delta`` / ``num_changes`` / ``change_rate`` and never updates them; this package does update them,
so the driver does too (a device scalar for delta, host numbers for the other two).

The JSON holds, per case: the recipe, the attribute names set_metrics created, the calls of every step (their array arguments by name in
the npz), and every key the wrap-up logged, in order, with its value, the count of the metric it came from, and ``{phase}/the_metric``.
Data only: no text of the reference is stored.

Usage:  python tools/gen_golden_epoch_metrics.py
"""
from __future__ import annotations

import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402,F401  (installs the stand-ins, imports the reference)


class Metric:
    """the part of Lightning's Metric the reference's four classes use"""

    def __init__(self, dist_sync_on_step=False):
        self._defaults = {}

    def add_state(self, name, default, dist_reduce_fx=None):
        self._defaults[name] = default.clone()
        setattr(self, name, default.clone())

    def reset(self):
        for name, default in self._defaults.items():
            setattr(self, name, default.clone())

    def __call__(self, *args, **kw):
        return self.update(*args, **kw)


def load_reference():
    import transformers.optimization as TO
    if not hasattr(TO, "AdamW"):
        TO.AdamW = torch.optim.AdamW
    sys.modules["pytorch_lightning.metrics"].Metric = Metric
    sys.modules["pytorch_lightning"].metrics.Metric = Metric
    import vilt.gadgets.my_metrics as ref_metrics      # noqa: F401  (reference, unmodified)
    import vilt.modules.vilt_utils as ref_utils        # (reference, unmodified)
    return ref_utils


class Stub:
    def __init__(self, loss_names, image_view, text_view, augmentation):
        self.hparams = types.SimpleNamespace(config={"loss_names": loss_names, "get_recall_metric": False})
        self.image_view, self.text_view, self.augmentation = image_view, text_view, augmentation
        self.training = True
        self.global_step = 0
        self.logged = []

    def log(self, name, value):
        self.logged.append((name, value))


ALL = ["moco", "barlowtwins", "itm", "mlm", "mpp", "vqa", "nlvr2", "irtr", "irtr_attacked", "nlvr2_attacked", "vqa_attacked"]

# (case, loss_names, image_view, text_view)
CASES = [("finetune_vqa", {"vqa": 1}, False, False),
         ("finetune_vqa_attacked_img", {"vqa_attacked": 1}, True, False),
         ("finetune_nlvr2", {"nlvr2": 1}, False, False),
         ("finetune_nlvr2_attacked_img", {"nlvr2_attacked": 1}, True, False),
         ("finetune_nlvr2_attacked_both", {"nlvr2_attacked": 1}, True, True),
         ("finetune_irtr", {"itm": 0.5, "irtr": 1}, False, False),
         ("mlm_itm", {"itm": 1, "mlm": 1}, False, False),
         ("mlm_itm_mpp", {"itm": 1, "mlm": 1, "mpp": 1}, False, False),
         ("moco_both", {"moco": 1}, True, True),
         ("barlowtwins_img", {"barlowtwins": 1}, True, False),
         ("barlowtwins_both", {"barlowtwins": 1}, True, True)]
STEPS = 4


class Recorder:
    """Feeds the stub's metric attributes and records every call: arrays go to the npz under `case/phase/step/n`"""

    def __init__(self, stub, arrays, prefix):
        self.stub, self.arrays, self.prefix, self.calls, self.n = stub, arrays, prefix, [], 0

    def _arg(self, v):
        if torch.is_tensor(v):
            key = f"{self.prefix}/{self.n}"
            self.n += 1
            self.arrays[key] = v.detach().numpy().copy()
            return {"npz": key}
        return {"host": float(v)}

    def call(self, attr, kind, *args, extra=None):
        getattr(self.stub, attr)(*args)
        c = {"attr": attr, "kind": kind, "args": [self._arg(a) for a in args]}
        if extra:
            c.update({k: self._arg(v) if torch.is_tensor(v) else v for k, v in extra.items()})
        self.calls.append(c)


def f32(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def loss_value(rng):
    return torch.tensor(np.float32(abs(rng.standard_normal()) + 0.3))


def feed_step(rec, rng, task, phase, step, image_view, text_view):
    if task in ("vqa", "vqa_attacked"):
        B, A = 5, 7
        logits = f32(rng, B, A)
        if step == 1:
            logits[0, 2] = logits[0, 5] = logits[0].max() + 1.0                # an exact tie: the first maximum scores
        targets = torch.from_numpy(rng.choice(np.array([0, 0, 0.3, 0.6, 0.9, 1.0], np.float32), size=(B, A)))
        rec.call(f"{phase}_{task}_score", "vqa", logits, targets)
        rec.call(f"{phase}_{task}_loss", "scalar", loss_value(rng))
    elif task in ("nlvr2", "nlvr2_attacked"):
        B = 6
        labels = torch.from_numpy(rng.integers(0, 2, B)).long()
        logits = f32(rng, B, 2)
        att = logits + f32(rng, B, 2, scale=0.8)
        views = image_view or text_view
        if phase == "train":
            if task == "nlvr2":
                rec.call("train_nlvr2_loss", "scalar", F.cross_entropy(logits, labels))
                rec.call("train_nlvr2_accuracy", "accuracy", logits, labels)
            else:
                rec.call("train_nlvr2_attacked_loss", "scalar", F.cross_entropy(att, labels))
                rec.call("train_nlvr2_attacked_accuracy", "accuracy", att, labels)
                if image_view:
                    rec.call("train_nlvr2_attacked_delta", "scalar", loss_value(rng) * 0.01)
                if text_view:
                    rec.call("train_nlvr2_attacked_num_changes", "scalar", float(rng.integers(0, 9)) / 4)
                    rec.call("train_nlvr2_attacked_change_rate", "scalar", float(rng.integers(0, 9)) / 32)
            return
        names = [("dev", "test", "dev", "dev", "test", "train")[(i + step) % 6] for i in range(B)]
        if step == 2:
            names = ["dev" if n == "test" else n for n in names]               # a validation batch without a test row
        group = torch.tensor([0 if "dev" in n else (1 if "test" in n else -1) for n in names], dtype=torch.int32)
        for g, split in enumerate(("dev", "test")):
            idx = [i for i, n in enumerate(names) if split in n]
            if not idx:
                continue
            for which, lg in ((("", logits),) if task == "nlvr2" else (("_original", logits),) + ((("_attacked", att),) if views else ())):
                rows = F.cross_entropy(lg, labels, reduction="none")
                rec.call(f"{split}_nlvr2{which}_loss", "scalar", F.cross_entropy(lg[idx], labels[idx]),
                         extra={"rowmean": True, "rows": rows, "group": group, "g": g})
                rec.call(f"{split}_nlvr2{which}_accuracy", "accuracy", lg[idx], labels[idx])
                if which == "_attacked":
                    rec.call(f"{split}_nlvr2_attacked_change_rate_cross", "change", att[idx], logits[idx])
    elif task == "irtr":
        rec.call(f"{phase}_irtr_loss", "scalar", loss_value(rng))
    elif task == "itm":
        B = 6
        labels = torch.from_numpy(rng.integers(0, 2, B)).long()
        rec.call(f"{phase}_itm_loss", "scalar", loss_value(rng))
        rec.call(f"{phase}_itm_wpa_loss", "scalar", loss_value(rng) * 0.1)
        rec.call(f"{phase}_itm_accuracy", "accuracy", f32(rng, B, 2), labels)
    elif task in ("mlm", "mpp"):
        shape, V = ((3, 8), 11) if task == "mlm" else ((2, 5, 3), 16)
        labels = torch.from_numpy(rng.integers(0, V, shape)).long()
        labels[torch.from_numpy(rng.random(shape) < 0.7)] = -100
        if task == "mlm" and phase == "val" and step == 1:
            labels[:] = -100                                                    # an MLM batch without a labelled row
        logits = f32(rng, *shape, V)
        # gate: the labelled rows of the batch (this package adds a batch's loss only when it has one; the reference adds the NaN)
        rec.call(f"{phase}_{task}_loss", "scalar", F.cross_entropy(logits.view(-1, V), labels.view(-1), ignore_index=-100),
                 extra={"gate": int((labels != -100).sum())})
        rec.call(f"{phase}_{task}_accuracy", "accuracy", logits, labels)
    elif task == "moco":
        rec.call(f"{phase}_moco_loss", "scalar", loss_value(rng) * 5)
    elif task == "barlowtwins":
        rec.call(f"{phase}_barlowtwins_loss", "scalar", loss_value(rng) * 100)
        for name in (["text"] if text_view else []) + (["img"] if image_view else []) + (["both"] if image_view and text_view else []):
            rec.call(f"{phase}_barlowtwins_loss_invariance_{name}", "scalar", loss_value(rng) * 60)
            rec.call(f"{phase}_barlowtwins_loss_redundancy_{name}", "scalar", loss_value(rng) * 40)
    else:
        raise ValueError(task)


def run():
    ref_utils = load_reference()
    arrays, cases = {}, []
    for ci, (name, ln, image_view, text_view) in enumerate(CASES):
        loss_names = {k: ln.get(k, 0) for k in ALL}
        stub = Stub(loss_names, image_view, text_view, False)
        before = set(vars(stub))
        ref_utils.set_metrics(stub)
        attrs = [a for a in vars(stub) if a not in before]
        case = {"name": name, "loss_names": loss_names, "image_view": image_view, "text_view": text_view, "augmentation": False,
                "attributes": attrs, "classes": {a: type(getattr(stub, a)).__name__ for a in attrs}, "phases": {}}
        for pi, phase in enumerate(("train", "val")):
            rng = np.random.default_rng(1000 * ci + pi)
            stub.training = phase == "train"
            steps = []
            for step in range(STEPS):
                rec = Recorder(stub, arrays, f"{name}/{phase}/{step}")
                for task, v in loss_names.items():
                    if v >= 1:
                        feed_step(rec, rng, task, phase, step, image_view, text_view)
                steps.append(rec.calls)
            # the count of every metric at the time of the wrap-up: tells a NaN of an empty metric (0 / 0) from a NaN addend
            totals = {a: float(getattr(stub, a).total) for a in attrs}
            stub.logged = []
            ref_utils.epoch_wrapup(stub)
            logged = [(k, float(v)) for k, v in stub.logged]
            assert logged[-1][0] == f"{phase}/the_metric"
            case["phases"][phase] = {
                "steps": steps, "totals": totals,
                "keys": [k for k, _ in logged[:-1]],
                "values": [None if math.isnan(v) else v for _, v in logged[:-1]],
                "the_metric": None if math.isnan(logged[-1][1]) else logged[-1][1]}
            print(name, phase, len(logged) - 1, "keys, the_metric", logged[-1][1])
        cases.append(case)
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "epoch_metrics.json"), "w") as f:
        json.dump({"steps": STEPS, "cases": cases}, f, indent=1)
    np.savez_compressed(os.path.join(gold, "epoch_metrics.npz"), **arrays)
    print("arrays", len(arrays), "bytes", os.path.getsize(os.path.join(gold, "epoch_metrics.npz")), os.path.getsize(os.path.join(gold, "epoch_metrics.json")))


if __name__ == "__main__":
    run()
