"""CPU: the epoch metrics against the reference's own metric classes, set_metrics and epoch_wrapup (tests/golden/epoch_metrics.json / .npz,
written by tools/gen_golden_epoch_metrics.py), with the numpy statement of the op kinds (tests/metrics_ref.py) standing in for the kernel.

The table of a recipe's epoch is formed by metrics_ref from the fixture's step inputs, through the ops the objectives queue, loaded into
a CPU ``EpochMetrics`` and wrapped up by ``vilt_utils.epoch_wrapup`` itself: key list and order, counts, epoch values and the_metric are the
package's own code path from the table on.  Also here: the host's argument checks of rmcl_metrics_update (they precede the launch, so
host buffers do), ``reduce_`` over two gloo ranks, the state round trip and the scratch-free ISA of csrc/metrics.hip."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd.vilt.gadgets import my_metrics
from rmcl_amd.vilt.modules import vilt_utils
from tests import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
U32 = 2.0 ** -24                       # unit roundoff of fp32: the reference's metric states are fp32 tensors

with open(os.path.join(GOLD, "epoch_metrics.json")) as _f:
    FIX = json.load(_f)
ARR = np.load(os.path.join(GOLD, "epoch_metrics.npz"))
CASES = {c["name"]: c for c in FIX["cases"]}


class Stub:
    """what set_metrics / epoch_wrapup read of a ViLTransformerSS"""

    def __init__(self, loss_names, image_view=False, text_view=False, augmentation=False, training=True):
        self.hparams = types.SimpleNamespace(config={"loss_names": dict(loss_names), "get_recall_metric": False})
        self.image_view, self.text_view, self.augmentation = image_view, text_view, augmentation
        self.training, self.logged, self.device, self.epoch_metrics = training, {}, torch.device("cpu"), None

    def log(self, name, value):
        self.logged[name] = value


def stub_of(case, phase):
    return Stub(case["loss_names"], case["image_view"], case["text_view"], case["augmentation"], training=phase == "train")


def arg(a):
    return ARR[a["npz"]] if "npz" in a else a["host"]


def apply_call(tab, slots, call, ref_chain):
    """One call of the reference's metric attribute as the op the objectives queue for it.  ref_chain[attr] collects what the bound on the
    reference's own fp32 arithmetic needs: (number of fp32 addends in its chain, sum of their magnitudes, slack of its step values)."""
    slot, kind, args = slots[call["attr"]], call["kind"], [arg(a) for a in call["args"]]
    n, mag, slack = ref_chain.setdefault(call["attr"], [0, 0.0, 0.0])[:3]
    if kind == "scalar" and call.get("gate") == 0:
        # a batch without a labelled row: the reference adds its NaN loss, the objectives gate the op on the row count
        R.apply(tab, R.SCALAR, slot, a=args[0], b=np.zeros(1, np.float32))
        ref_chain[call["attr"]][3:] = [True]
        return
    if kind == "scalar":
        if call.get("rowmean"):
            # the validation split's mean CE: the reference feeds the fp32 mean of the split's rows, the objectives queue ROWMEAN on
            # the per-row CE with the split as the group
            rows, g = ARR[call["rows"]["npz"]], ARR[call["group"]["npz"]]
            group = np.where(g == call["g"], 0, -1).astype(np.int32)
            R.apply(tab, R.ROWMEAN, slot, a=rows, rows=len(rows), group=group)
            mine = np.abs(rows[group == 0].astype(np.float64))
            slack += (len(mine) + 1) * U32 * float(mine.sum()) / len(mine)   # its serial fp32 sum of n_g rows, then the division
            x = float(np.float32(args[0]))
        elif isinstance(args[0], float):
            R.apply(tab, R.SCALAR, slot, imm=args[0])
            x = float(np.float32(args[0]))
        else:
            R.apply(tab, R.SCALAR, slot, a=args[0])
            x = float(args[0])
        n, mag = n + 1, mag + (abs(x) if not math.isnan(x) else 0.0)
    elif kind == "accuracy":
        logits, labels = args
        V = logits.shape[-1]
        R.apply(tab, R.ARGMAX_MATCH, slot, a=logits.reshape(-1, V), b=labels.reshape(-1), rows=labels.size, ncols=V)
    elif kind == "vqa":
        logits, targets = args
        picked = targets[np.arange(len(logits)), R.argmax_first(logits)].astype(np.float32)      # rows[:, 1] of rmcl_vqa_bce
        R.apply(tab, R.ROWSUM, slot, a=picked, rows=len(picked))
        n, mag = n + len(picked), mag + float(np.abs(picked.astype(np.float64)).sum())
    elif kind == "change":
        la, lo = args
        R.apply(tab, R.MATCH, slot, a=R.argmax_first(la), b=R.argmax_first(lo), rows=len(la), flags=R.INVERT)
    else:
        raise ValueError(kind)
    ref_chain[call["attr"]][:3] = [n, mag, slack]


def wrapped_up(case, phase):
    """(stub after epoch_wrapup, RefTable, ref_chain, slots) of one fixture epoch"""
    stub = stub_of(case, phase)
    em = vilt_utils.set_metrics(stub)
    tab, chain = R.RefTable(len(em.slots)), {}
    for calls in case["phases"][phase]["steps"]:
        for call in calls:
            apply_call(tab, em.slots, call, chain)
    em.table.copy_(torch.from_numpy(tab.t))
    vilt_utils.epoch_wrapup(stub)
    return stub, tab, chain, dict(em.slots)


PARAMS = [(c["name"], ph) for c in FIX["cases"] for ph in ("train", "val")]


@pytest.mark.parametrize("name", sorted(CASES))
def test_set_metrics_creates_the_reference_attributes(name):
    case = CASES[name]
    stub = stub_of(case, "train")
    before = set(vars(stub))
    vilt_utils.set_metrics(stub)
    made = [a for a in vars(stub) if a not in before and a != "epoch_metrics"]
    assert made == case["attributes"]                                         # the names, in the reference's creation order
    assert {a: type(getattr(stub, a)).__name__ for a in made} == case["classes"]
    assert [a for a, _ in vilt_utils.metric_attributes(case["loss_names"], case["image_view"], case["text_view"])] == case["attributes"]


@pytest.mark.parametrize("name,phase", PARAMS)
def test_epoch_keys_and_values_match_the_reference(name, phase):
    case = CASES[name]
    fx = case["phases"][phase]
    stub, tab, chain, slots = wrapped_up(case, phase)
    out = stub.last_epoch_metrics
    assert out["phase"] == phase
    mine = [k for k in out if k not in ("phase", f"{phase}/the_metric")]
    # every key the reference logged with a value, in its order - and nothing else; a key it logged as NaN is absent here when the metric
    # is empty (0 / 0), and finite when the NaN was the loss of a batch without a labelled row (checked below)
    assert [k for k in fx["keys"] if k in out] == mine and all(math.isfinite(out[k]) for k in mine)
    assert [k for k, v in zip(fx["keys"], fx["values"]) if v is not None] == [k for k in mine if fx["values"][fx["keys"].index(k)] is not None]
    plan = {key: (attr, shown, is_value) for _, es in vilt_utils.epoch_plan(case["loss_names"], phase, case["image_view"], case["text_view"])
            for key, attr, shown, is_value in es}
    worst, bounds = 0.0, {}
    for key, want in zip(fx["keys"], fx["values"]):
        attr, shown, _ = plan[key]
        if want is None:
            if key in out:
                # the reference's NaN comes from the NaN loss of a batch without a labelled row: here that batch is left out, and the
                # epoch value is the mean over the others
                gated = len(chain[shown]) > 3
                assert gated and 0 < tab.t[slots[shown], 1] < fx["totals"][shown] and math.isfinite(out[key]), key
                assert out[key] == tab.t[slots[shown], 0] / tab.t[slots[shown], 1], key
            else:
                assert fx["totals"][shown] == 0, key
            continue
        got = out[key]
        count = tab.t[slots[shown], 1]
        assert count == fx["totals"][shown], (key, count)                     # counts are exact
        if case["classes"][shown] in ("Accuracy", "change_rate"):
            assert float(np.float32(got)) == want, (key, got, want)           # integer / integer: equal once rounded to the reference's fp32
            bounds[key] = U32 * abs(want)
            continue
        # the reference adds its n fp32 addends one after the other in fp32: |error| <= (n - 1) u sum|x|, then one rounding of the quotient;
        # `slack`: the rounding already in the step values it fed (the fp32 mean of a split's rows)
        n, mag, slack = chain[shown][:3]
        bound = ((n - 1) * U32 * mag + slack) / count + U32 * abs(want) + tab.bound(slots[shown]) / count
        assert abs(got - want) <= bound, (key, got, want, bound)
        bounds[key] = bound
        worst = max(worst, abs(got - want) / bound)
    print(f"{name}/{phase}: largest |epoch value - reference| / bound = {worst:.3f}")
    values = [key for key in fx["keys"] if plan[key][2]]
    last = {}                                                                 # the LAST value key of each task joins the_metric
    for key in values:
        last[[t for t, es in vilt_utils.epoch_plan(case["loss_names"], phase, case["image_view"], case["text_view"])
              if any(e[0] == key for e in es)][0]] = key
    if fx["the_metric"] is None or any(k not in bounds for k in last.values()):
        assert f"{phase}/the_metric" not in out
    else:
        # its sum runs in fp32 too: one rounding per term on top of the terms' own bounds
        tol = sum(bounds[k] for k in last.values()) + len(last) * U32 * abs(fx["the_metric"])
        assert abs(out[f"{phase}/the_metric"] - fx["the_metric"]) <= tol, (out[f"{phase}/the_metric"], fx["the_metric"], tol)
    # the slots of the phase are reset, the others untouched
    assert float(stub.epoch_metrics.table.abs().sum()) == 0.0


def test_imitated_quirks():
    """The surprising cases of the reference's `value`, by name (DESIGN.md "Epoch metrics")."""
    moco = wrapped_up(CASES["moco_both"], "val")[0].last_epoch_metrics
    assert moco["val/the_metric"] == moco["moco_loss/epoch/val"]              # the LOSS, under mode max
    bt = wrapped_up(CASES["barlowtwins_both"], "train")[0].last_epoch_metrics
    assert bt["train/the_metric"] == bt["barlowtwins_loss/epoch/train"]
    assert bt["barlowtwins_loss_redundancy_both/epoch/train"] == bt["barlowtwins_loss_redundancy_text/epoch/train"]   # (:298)
    nl = wrapped_up(CASES["finetune_nlvr2_attacked_img"], "val")[0].last_epoch_metrics
    assert nl["val/the_metric"] == nl["nlvr2_attacked/test/change_rate_cross_epoch"]
    assert wrapped_up(CASES["finetune_irtr"], "val")[0].last_epoch_metrics["val/the_metric"] == 0.0
    stub, tab, _, slots = wrapped_up(CASES["mlm_itm"], "val")
    fx = CASES["mlm_itm"]["phases"]["val"]
    assert fx["values"][fx["keys"].index("mlm/val/loss_epoch")] is None       # an all-ignored MLM batch: NaN in the reference's epoch loss,
    assert math.isfinite(stub.last_epoch_metrics["mlm/val/loss_epoch"])       # left out here: the mean over the labelled batches
    assert tab.t[slots["val_mlm_loss"], 1] == FIX["steps"] - 1


def test_empty_slots_give_no_key_and_no_the_metric():
    stub = Stub({"nlvr2": 1}, training=False)
    em = vilt_utils.set_metrics(stub)
    em.table[em.slots["dev_nlvr2_accuracy"]] = torch.tensor([3.0, 4.0], dtype=torch.float64)
    em.table[em.slots["dev_nlvr2_loss"]] = torch.tensor([1.5, 2.0], dtype=torch.float64)
    out = vilt_utils.epoch_wrapup(stub)
    assert out == {"phase": "val", "nlvr2/dev/accuracy_epoch": 0.75, "nlvr2/dev/loss_epoch": 0.75}     # no test key, no val/the_metric
    em.table[em.slots["test_nlvr2_accuracy"]] = torch.tensor([1.0, 4.0], dtype=torch.float64)
    out = vilt_utils.epoch_wrapup(stub)
    assert out == {"phase": "val", "nlvr2/test/accuracy_epoch": 0.25, "val/the_metric": 0.25}          # the LAST value the task assigns
    assert all(math.isfinite(v) for k, v in out.items() if k != "phase")


def test_a_logged_the_metric_wins_and_the_bare_key_stays_out():
    stub = Stub({"vqa": 1}, training=False)
    em = vilt_utils.set_metrics(stub)
    em.table[em.slots["val_vqa_score"]] = torch.tensor([2.0, 4.0], dtype=torch.float64)
    stub.log("val/the_metric", 0.7)
    out = vilt_utils.epoch_wrapup(stub)
    assert out["val/the_metric"] == 0.7 and out["vqa/val/score_epoch"] == 0.5 and "the_metric" not in out
    assert list(out)[:2] == ["phase", "val/the_metric"]


def test_without_set_metrics_the_wrap_up_returns_what_it_did():
    stub = Stub({"vqa": 1}, training=False)
    stub.log("vqa/val/loss", torch.tensor(1.25))
    assert vilt_utils.epoch_wrapup(stub) == {"phase": "val", "vqa/val/loss": 1.25}


def test_handles_and_state_round_trip():
    stub = Stub({"itm": 1, "mlm": 1})
    em = vilt_utils.set_metrics(stub)
    assert math.isnan(stub.train_itm_accuracy.compute())                      # the reference's 0 / 0
    em.table[em.slots["train_itm_accuracy"]] = torch.tensor([5.0, 8.0], dtype=torch.float64)
    em.table[em.slots["val_mlm_loss"]] = torch.tensor([0.1 + 0.2, 3.0], dtype=torch.float64)
    assert stub.train_itm_accuracy.compute() == 0.625
    sd = em.state_dict()
    other = vilt_utils.set_metrics(Stub({"mlm": 1, "itm": 1, "mpp": 1}))      # another registry order: states travel by name
    other.load_state_dict(sd)
    assert other.pairs()["train_itm_accuracy"] == (5.0, 8.0) and other.pairs()["val_mlm_loss"] == (0.1 + 0.2, 3.0)
    assert other.pairs()["train_mpp_loss"] == (0.0, 0.0)
    other.load_state_dict(None)                                               # a training state without the key: an empty table
    assert float(other.table.abs().sum()) == 0.0
    stub.train_itm_accuracy.reset()
    assert em.pairs()["train_itm_accuracy"] == (0.0, 0.0) and em.pairs()["val_mlm_loss"][1] == 3.0
    with pytest.raises(RuntimeError, match="GPU"):
        stub.train_itm_loss.update(1.0)                                       # updates need the device


def _reduce_worker(rank, world, initfile, out_dir):
    import torch.distributed as dist
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.vilt.modules import vilt_utils as VU
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    stub = Stub({"vqa": 1, "itm": 1}, training=False)
    em = VU.set_metrics(stub)
    g = torch.Generator().manual_seed(17 + rank)
    em.table.copy_(torch.rand(em.table.shape, generator=g, dtype=torch.float64))
    torch.save(em.table.clone(), os.path.join(out_dir, f"own{rank}.pt"))
    em.reduce_()
    torch.save(em.table.clone(), os.path.join(out_dir, f"sum{rank}.pt"))
    dist.destroy_process_group()


def test_reduce_sums_the_table_over_two_gloo_ranks():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_reduce_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        own = [torch.load(os.path.join(d, f"own{r}.pt")) for r in range(2)]
        got = [torch.load(os.path.join(d, f"sum{r}.pt")) for r in range(2)]
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], own[0] + own[1])          # the one-process table of both ranks' updates
    em = my_metrics.EpochMetrics("cpu")
    em.register("a")
    em.table[0] = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert em.reduce_() is em and em.pairs()["a"] == (1.0, 2.0)                          # no process group: nothing happens


# ---- the host's checks of rmcl_metrics_update: they precede the launch, host buffers do --------------------------------------------------
def _ops(*ops):
    o = L.MetricOps(n_ops=len(ops))
    for i, f in enumerate(ops[:L.METRIC_MAX_OPS]):
        o.op[i] = L.MetricOp(**f)
    return o


def test_rejected_calls_launch_nothing():
    lib = L.lib
    table = (C.c_double * 16)(*range(16))
    before = bytes(table)
    buf, ibuf = (C.c_float * 16)(), (C.c_int32 * 16)()
    a, ia = C.addressof(buf), C.addressof(ibuf)
    ok = dict(kind=L.METRIC_SCALAR, slot=0, n_groups=1, scale=1.0)
    bad = {
        "no ops": _ops(),
        "nine ops": L.MetricOps(n_ops=9),
        "unknown kind": _ops(dict(ok, kind=6)),
        "unknown flag": _ops(dict(ok, flags=2)),
        "slot behind the table": _ops(dict(ok, slot=8)),
        "negative slot": _ops(dict(ok, slot=-1)),
        "group range behind the table": _ops(dict(kind=L.METRIC_ROWSUM, slot=6, n_groups=3, rows=1, stride=1, a=a)),
        "no groups": _ops(dict(ok, n_groups=0)),
        "five groups": _ops(dict(kind=L.METRIC_ROWSUM, slot=0, n_groups=5, rows=1, stride=1, a=a)),
        "negative rows": _ops(dict(kind=L.METRIC_ROWSUM, slot=0, n_groups=1, rows=-1, stride=1, a=a)),
        "zero stride": _ops(dict(kind=L.METRIC_ROWMEAN, slot=0, n_groups=1, rows=1, stride=0, a=a)),
        "pair without den": _ops(dict(kind=L.METRIC_PAIR, slot=0, n_groups=1, a=a)),
        "rowsum without x": _ops(dict(kind=L.METRIC_ROWSUM, slot=0, n_groups=1, rows=1, stride=1)),
        "match without b": _ops(dict(kind=L.METRIC_MATCH, slot=0, n_groups=1, rows=1, a=ia)),
        "argmax without logits": _ops(dict(kind=L.METRIC_ARGMAX_MATCH, slot=0, n_groups=1, rows=1, ncols=2, pitch=2, b=ia)),
        "no columns": _ops(dict(kind=L.METRIC_ARGMAX_MATCH, slot=0, n_groups=1, rows=1, ncols=0, pitch=2, a=a, b=ia)),
        "columns past the pitch": _ops(dict(kind=L.METRIC_ARGMAX_MATCH, slot=0, n_groups=1, rows=1, ncols=3, pitch=2, a=a, b=ia)),
        "shared slot": _ops(ok, dict(ok, slot=1), dict(ok, slot=0)),
        "overlapping group ranges": _ops(dict(kind=L.METRIC_ROWSUM, slot=0, n_groups=2, rows=1, stride=1, a=a), dict(ok, slot=1)),
    }
    for what, ops in bad.items():
        assert lib.rmcl_metrics_update(table, 8, C.byref(ops), None) == -1, what
        assert b"metrics_update" in lib.rmcl_last_error(), what
        assert bytes(table) == before, what
    assert lib.rmcl_metrics_update(None, 8, C.byref(_ops(ok)), None) == -1 and b"NULL" in lib.rmcl_last_error()
    assert lib.rmcl_metrics_update(table, 8, None, None) == -1 and b"NULL" in lib.rmcl_last_error()
    assert lib.rmcl_metrics_update(table, 0, C.byref(_ops(ok)), None) == -1
    assert C.sizeof(L.MetricOp) == 72 and C.sizeof(L.MetricOps) == 8 + 8 * 72          # the layout of include/rmcl.h


def test_flush_splits_launches_at_eight_ops_and_at_shared_slots(monkeypatch):
    em = my_metrics.EpochMetrics("cpu")
    for i in range(12):
        em.register(f"m{i}")
    em.device = torch.device("cuda")                                          # (queueing only: the launch is replaced below)
    seen = []
    monkeypatch.setattr(L.lib, "rmcl_metrics_update", lambda t, n, ops, s: seen.append([ops._obj.op[i].slot for i in range(ops._obj.n_ops)]) or 0)
    from rmcl_amd import runtime
    monkeypatch.setattr(runtime, "stream_ptr", lambda: None)
    for i in list(range(10)) + [9, 3]:
        em.scalar(f"m{i}", 1.0)
    em.flush()
    assert seen == [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9], [9, 3]] and em.pending == []


# ---- ISA: no scratch ---------------------------------------------------------------------------------------------------------------------
def test_metrics_kernel_uses_no_scratch():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    src = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc", "metrics.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only",
             "-I" + os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "metrics.s")
        r = subprocess.run(["hipcc", *flags, src, "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        isa = open(dst).read()
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    assert any("metrics_update_kernel" in n for n, _ in sizes), sizes
    assert not [(n[:80], int(s)) for n, s in sizes if int(s) != 0], sizes
    assert "global_atomic" not in isa and "flat_atomic" not in isa and "ds_add" not in isa           # no atomics of any kind
