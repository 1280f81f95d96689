"""The reference's epoch metrics (vilt/gadgets/my_metrics.py: Accuracy, VQAScore, Scalar, change_rate) on ONE device table.

Each of the reference's four classes keeps a (sum, count) pair and divides at the end of the epoch.  ``EpochMetrics`` keeps every pair of a
model in one ``double [n_slots][2]`` tensor; a step *queues* additions (``scalar`` / ``pair`` / ``rowsum`` / ``rowmean`` / ``match`` /
``argmax_match``, the op kinds of include/rmcl.h ``rmcl_metrics_update``) on buffers the step's kernels already wrote, and ``flush()`` sends
them as one launch per eight ops - no synchronisation, no copy to the host, no torch launch per metric.  ``compute`` / ``reset`` /
``state_dict`` / ``reduce_`` read or write the table and are for epoch ends; they work on a CPU table too (updates need the GPU).

The classes at the bottom are the handles ``vilt_utils.set_metrics`` hangs on the module under the reference's attribute names: the
reference's ``compute()`` / ``reset()`` / ``update(...)`` / ``__call__`` surface over a slot of the table."""
from __future__ import annotations

import ctypes as C

import torch

from ... import _lib as L


def _ptr(t, dtype, what):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda:
        raise TypeError(f"EpochMetrics: {what} must be a {dtype} tensor on the GPU (got {type(t).__name__}"
                        f"{'' if not torch.is_tensor(t) else f' {t.dtype} on {t.device}'})")
    return t.data_ptr()


class EpochMetrics:
    def __init__(self, device):
        self.device = torch.device(device)
        self.slots = {}                                         # name -> slot
        self.table = torch.zeros(0, 2, dtype=torch.float64, device=self.device)
        self.pending = []                                       # (MetricOp, first slot, slots, tensors kept alive until the launch)

    # ---- registry ----------------------------------------------------------------------------------------------------------------
    def register(self, *names):
        """Slots for `names`, consecutive and in this order when none of them exists yet (what a grouped op needs); returns the first."""
        new = [n for n in names if n not in self.slots]
        if new and len(new) != len(names):
            raise ValueError(f"EpochMetrics.register: {names} mixes registered and new names")
        if new:
            base = len(self.slots)
            for i, n in enumerate(names):
                self.slots[n] = base + i
            self.table = torch.cat([self.table, torch.zeros(len(names), 2, dtype=torch.float64, device=self.device)])
        return self.slots[names[0]]

    def _range(self, names):
        names = [names] if isinstance(names, str) else list(names)
        s = [self.slots[n] for n in names]
        if s != list(range(s[0], s[0] + len(s))):
            raise ValueError(f"EpochMetrics: the slots of {names} are not consecutive (register them in one call)")
        if len(s) > L.METRIC_MAX_GROUPS:
            raise ValueError(f"EpochMetrics: at most {L.METRIC_MAX_GROUPS} groups per op")
        return s[0], len(s)

    # ---- queueing (GPU only) -----------------------------------------------------------------------------------------------------
    def _queue(self, names, keep, **fields):
        slot, n = self._range(names)
        if self.device.type != "cuda":
            raise RuntimeError("EpochMetrics: updates run on the GPU (rmcl_metrics_update); a CPU table only computes, reduces and stores")
        op = L.MetricOp(slot=slot, n_groups=n, **fields)
        self.pending.append((op, slot, n, keep))

    def scalar(self, name, x, scale=1.0, gate=None):
        """Scalar.update: sum += scale * x, count += 1; x a one-element fp32 device tensor, or a host number (sent as an immediate).
        gate: a one-element fp32 device tensor; the op adds nothing when it holds 0 (a count of labelled rows)"""
        g = None if gate is None else _ptr(gate, torch.float32, "gate")
        if torch.is_tensor(x):
            self._queue(name, (x, gate), kind=L.METRIC_SCALAR, scale=scale, a=_ptr(x, torch.float32, "a scalar"), b=g)
        else:
            self._queue(name, (gate,), kind=L.METRIC_SCALAR, scale=scale, imm=float(x), a=None, b=g)

    def pair(self, name, num, den):
        self._queue(name, (num, den), kind=L.METRIC_PAIR, a=_ptr(num, torch.float32, "num"), b=_ptr(den, torch.float32, "den"))

    def _rows(self, kind, names, x, rows, stride, group):
        g = None if group is None else _ptr(group, torch.int32, "group")
        self._queue(names, (x, group), kind=kind, rows=int(rows), stride=int(stride), a=_ptr(x, torch.float32, "x"), group=g)

    def rowsum(self, names, x, rows, stride=1, group=None):
        self._rows(L.METRIC_ROWSUM, names, x, rows, stride, group)

    def rowmean(self, names, x, rows, stride=1, group=None):
        self._rows(L.METRIC_ROWMEAN, names, x, rows, stride, group)

    def match(self, names, a, b, rows, ignore_index=-100, invert=False, group=None):
        g = None if group is None else _ptr(group, torch.int32, "group")
        self._queue(names, (a, b, group), kind=L.METRIC_MATCH, rows=int(rows), ignore_index=int(ignore_index),
                    flags=L.METRIC_INVERT if invert else 0, a=_ptr(a, torch.int32, "a"), b=_ptr(b, torch.int32, "b"), group=g)

    def argmax_match(self, names, logits, labels, ignore_index=-100, invert=False, group=None):
        """logits: fp32 [rows, ncols], rows at any pitch (stride(1) == 1)"""
        if logits.dim() != 2 or logits.stride(1) != 1:
            raise ValueError("EpochMetrics.argmax_match: logits must be [rows, ncols] with unit column stride")
        g = None if group is None else _ptr(group, torch.int32, "group")
        rows, ncols = int(logits.shape[0]), int(logits.shape[1])
        self._queue(names, (logits, labels, group), kind=L.METRIC_ARGMAX_MATCH, rows=rows, ncols=ncols,
                    pitch=int(logits.stride(0)) if rows > 1 else ncols, ignore_index=int(ignore_index),
                    flags=L.METRIC_INVERT if invert else 0, a=_ptr(logits, torch.float32, "logits"),
                    b=_ptr(labels, torch.int32, "labels"), group=g)

    def flush(self):
        """The queued ops as rmcl_metrics_update launches on the current stream: eight ops per launch, and a new launch wherever an op
        touches a slot an earlier op of the launch owns (the workgroups of one launch run concurrently)."""
        if not self.pending:
            return
        from ...runtime import stream_ptr
        pending, self.pending = self.pending, []
        batch, owned = [], set()

        def launch():
            ops = L.MetricOps(n_ops=len(batch))
            for i, op in enumerate(batch):
                ops.op[i] = op
            L.check(L.lib.rmcl_metrics_update(self.table.data_ptr(), int(self.table.shape[0]), C.byref(ops), stream_ptr()), "metrics_update")

        for op, slot, n, _keep in pending:
            mine = set(range(slot, slot + n))
            if len(batch) == L.METRIC_MAX_OPS or owned & mine:
                launch()
                batch, owned = [], set()
            batch.append(op)
            owned |= mine
        launch()

    # ---- epoch ends ----------------------------------------------------------------------------------------------------------------
    def pairs(self):
        """{name: (sum, count)} of the whole table in one read (synchronises)"""
        self.flush()
        host = self.table.detach().cpu().tolist()
        return {n: tuple(host[s]) for n, s in self.slots.items()}

    def compute(self, name):
        """sum / count of the slot (synchronises); NaN for a slot that received nothing, like the reference's 0 / 0"""
        self.flush()
        s, c = self.table[self.slots[name]].tolist()
        return s / c if c else float("nan")

    def reset(self, name=None):
        self.flush()
        if name is None:
            self.table.zero_()
        else:
            self.table[self.slots[name]].zero_()

    def reduce_(self, group=None):
        """Lightning's dist_reduce_fx="sum" at compute(): ONE all-reduce of the whole table when a process group with more than one rank
        is initialised, nothing otherwise.  Every rank must call it with the same registry."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) < 2:
            return self
        self.flush()
        dist.all_reduce(self.table, op=dist.ReduceOp.SUM, group=group)
        return self

    def state_dict(self):
        self.flush()
        return {"names": list(self.slots), "table": self.table.detach().cpu().clone()}

    def load_state_dict(self, sd):
        """By name: a name the state does not know keeps an empty slot, a name this table does not know is dropped.  None / {}: empty."""
        self.pending = []
        self.table.zero_()
        if not sd:
            return
        host = torch.zeros(len(self.slots), 2, dtype=torch.float64)
        for i, n in enumerate(sd["names"]):
            if n in self.slots:
                host[self.slots[n]] = sd["table"][i].to(torch.float64)
        self.table.copy_(host)


# ---- the reference's classes as handles on a slot --------------------------------------------------------------------------------------
class _Handle:
    def __init__(self, metrics: EpochMetrics, name: str):
        self.metrics, self.name = metrics, name
        if name not in metrics.slots:
            metrics.register(name)

    def compute(self):
        return self.metrics.compute(self.name)

    def reset(self):
        self.metrics.reset(self.name)

    def __call__(self, *args, **kw):
        """Queues the update and sends it; unlike the reference's forward it returns nothing (a step value would synchronise)"""
        self.update(*args, **kw)
        self.metrics.flush()


class Scalar(_Handle):
    def update(self, scalar, scale=1.0, gate=None):
        self.metrics.scalar(self.name, scalar.detach() if torch.is_tensor(scalar) else scalar, scale, gate)


class Accuracy(_Handle):
    def update(self, logits, target):
        """fp32 logits [rows, ncols] against int32 labels (rows whose label is -100 are left out); other label types are cast"""
        target = target if target.dtype == torch.int32 else target.to(torch.int32)
        self.metrics.argmax_match(self.name, logits.detach(), target)

    def update_match(self, pred, target, rows=None):
        self.metrics.match(self.name, pred, target, int(pred.numel()) if rows is None else rows)

    def update_counts(self, correct, total):
        self.metrics.pair(self.name, correct, total)


class VQAScore(_Handle):
    def update(self, scores, rows, stride=1):
        """scores[r * stride] = the soft target at the first maximum of row r's logits: rows[:, 1] of rmcl_vqa_bce, which has already
        done the reference's argmax / one-hot / product (the reference's update takes the logits and the targets)"""
        self.metrics.rowsum(self.name, scores, rows, stride)


class change_rate(_Handle):                                    # (the reference's spelling)
    def update(self, pred_attack, pred, rows=None, group=None):
        """int32 argmax of the attacked pass against the clean pass's (the reference's update takes both logits)"""
        self.metrics.match(self.name, pred_attack, pred, int(pred.numel()) if rows is None else rows, invert=True, group=group)
