"""Training utilities on the hot path's edge: ``set_task`` (vilt/modules/vilt_utils.py:325-329) and
``set_schedule`` (:331-437) = HF AdamW (beta (0.9,0.98), eps 1e-8, 4 parameter groups) + polynomial
decay with warm-up, restated as ONE fused multi-tensor kernel over the flat parameter arena.  ``optim_type`` "adam" and "sgd"
(:399-402) are the same object over another update rule: FusedAdam, FusedSGD."""
from __future__ import annotations

import ctypes as C
import math

import torch

from ... import _lib as L
from ..._lib import lib, check, P, I64, F
from ...runtime import stream_ptr
from . import schedules

NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight", "norm.bias", "norm.weight", "norm1.bias", "norm1.weight",
            "norm2.bias", "norm2.weight"]
HEAD_NAMES = ["vqa_classifier", "nlvr2_classifier", "moco_head", "barlowtwinshead"]


def set_task(pl_module):
    pl_module.current_tasks = [k for k, v in pl_module.hparams.config["loss_names"].items() if v >= 1]
    return


def _views(pl_module):
    return (bool(getattr(pl_module, "image_view", False)), bool(getattr(pl_module, "text_view", False)),
            bool(getattr(pl_module, "augmentation", False)))


def metric_attributes(loss_names, image_view=False, text_view=False, augmentation=False):
    """[(attribute name, class name)] of vilt_utils.set_metrics (:13-84), in its order, under its conditions.  ``irtr_attacked`` is
    broken upstream and not built here: it gets no attribute."""
    out = []
    add = lambda name, cls: out.append((name, cls))
    for split in ("train", "val"):
        for k, v in loss_names.items():
            if v < 1 or k == "irtr_attacked":
                continue
            if k in ("vqa", "vqa_attacked"):
                add(f"{split}_{k}_score", "VQAScore")
                add(f"{split}_{k}_loss", "Scalar")
            elif k == "nlvr2":
                for s in (("train",) if split == "train" else ("dev", "test")):
                    add(f"{s}_nlvr2_accuracy", "Accuracy")
                    add(f"{s}_nlvr2_loss", "Scalar")
            elif k == "nlvr2_attacked":
                if split == "train":
                    add(f"train_{k}_accuracy", "Accuracy")
                    add(f"train_{k}_loss", "Scalar")
                    if image_view:
                        add(f"train_{k}_delta", "Scalar")
                    if text_view:
                        add(f"train_{k}_num_changes", "Scalar")
                        add(f"train_{k}_change_rate", "Scalar")
                else:
                    for s in ("dev", "test"):
                        for which in ("original", "attacked"):
                            add(f"{s}_nlvr2_{which}_accuracy", "Accuracy")
                            add(f"{s}_nlvr2_{which}_loss", "Scalar")
                    add("test_nlvr2_attacked_change_rate_cross", "change_rate")
                    add("dev_nlvr2_attacked_change_rate_cross", "change_rate")
            elif k == "irtr":
                add(f"{split}_irtr_loss", "Scalar")
            elif k in ("mppd", "mpfr"):
                add(f"{split}_{k}_loss", "Scalar")
            elif k == "itm":
                add(f"{split}_itm_accuracy", "Accuracy")
                add(f"{split}_itm_loss", "Scalar")
                add(f"{split}_itm_wpa_loss", "Scalar")
            elif k in ("moco", "barlowtwins"):
                add(f"{split}_{k}_loss", "Scalar")
                if k == "barlowtwins":
                    names = (["img"] if image_view else []) + (["text"] if text_view else []) + \
                            (["both"] if image_view and text_view and not augmentation else [])
                    for n in names:
                        add(f"{split}_{k}_loss_invariance_{n}", "Scalar")
                        add(f"{split}_{k}_loss_redundancy_{n}", "Scalar")
            else:
                add(f"{split}_{k}_accuracy", "Accuracy")
                add(f"{split}_{k}_loss", "Scalar")
    return out


def set_metrics(pl_module):
    """vilt_utils.set_metrics (:13-84): the reference's metric attributes under its names, as handles on the slots of ONE device table,
    ``pl_module.epoch_metrics`` (vilt/gadgets/my_metrics.py).  The dev / test twins of NLVR2 get neighbouring slots: one grouped op
    serves both splits of a validation batch."""
    from ..gadgets import my_metrics
    image_view, text_view, augmentation = _views(pl_module)
    em = my_metrics.EpochMetrics(pl_module.device)
    attrs = metric_attributes(pl_module.hparams.config["loss_names"], image_view, text_view, augmentation)
    names = [n for n, _ in attrs]
    for name in names:
        if name.startswith("dev_") and "test_" + name[4:] in names:
            em.register(name, "test_" + name[4:])
    for name, cls in attrs:
        setattr(pl_module, name, getattr(my_metrics, cls)(em, name))
    pl_module.epoch_metrics = em
    return em


def epoch_plan(loss_names, phase, image_view=False, text_view=False, augmentation=False):
    """What vilt_utils.epoch_wrapup (:98-311) logs for `phase`, task by task in dict order: [(task, [(key, attribute, shown, is_value)])].
    ``attribute`` is computed and reset; the logged value is the one of ``shown`` (the reference logs the TEXT redundancy under
    redundancy_both, :298); the LAST entry with ``is_value`` is the task's term of the_metric, 0 when there is none (IRTR)."""
    plan = []
    for k, v in loss_names.items():
        if v < 1 or k == "irtr_attacked":
            continue
        e = []
        add = lambda key, attr, is_value=False, shown=None: e.append((key, attr, shown or attr, is_value))
        if k in ("vqa", "vqa_attacked"):
            add(f"{k}/{phase}/score_epoch", f"{phase}_{k}_score", True)
            add(f"{k}/{phase}/loss_epoch", f"{phase}_{k}_loss")
        elif k == "nlvr2":
            for s in (("train",) if phase == "train" else ("dev", "test")):
                add(f"nlvr2/{s}/accuracy_epoch", f"{s}_nlvr2_accuracy", True)
                add(f"nlvr2/{s}/loss_epoch", f"{s}_nlvr2_loss")
        elif k == "nlvr2_attacked":
            if phase == "train":
                add(f"{k}/train/accuracy_epoch", f"train_{k}_accuracy", True)
                add(f"{k}/train/loss_epoch", f"train_{k}_loss")
                if image_view:
                    add(f"{k}/train/img_delta_epoch", f"train_{k}_delta", True)
                if text_view:
                    add(f"{k}/train/txt_num_changes", f"train_{k}_num_changes", True)
                    add(f"{k}/train/txt_change_rate", f"train_{k}_change_rate", True)
            else:
                for s in ("dev", "test"):
                    add(f"nlvr2_original/{s}/accuracy_epoch", f"{s}_nlvr2_original_accuracy", True)
                    add(f"nlvr2_original/{s}/loss_epoch", f"{s}_nlvr2_original_loss")
                    if image_view or text_view:
                        add(f"nlvr2_attacked/{s}/accuracy_epoch", f"{s}_nlvr2_attacked_accuracy", True)
                        add(f"nlvr2_attacked/{s}/loss_epoch", f"{s}_nlvr2_attacked_loss")
                        add(f"nlvr2_attacked/{s}/change_rate_cross_epoch", f"{s}_nlvr2_attacked_change_rate_cross", True)
        elif k == "irtr":
            add(f"irtr/{phase}/irtr_loss_epoch", f"{phase}_irtr_loss")
        elif k in ("mppd", "mpfr"):
            add(f"{k}/{phase}/loss_epoch", f"{phase}_{k}_loss")
        elif k == "itm":
            add(f"itm/{phase}/accuracy_epoch", f"{phase}_itm_accuracy", True)
            add(f"itm/{phase}/loss_epoch", f"{phase}_itm_loss")
            add(f"itm/{phase}/wpa_loss_epoch", f"{phase}_itm_wpa_loss")
        elif k in ("moco", "barlowtwins"):
            add(f"{k}_loss/epoch/{phase}", f"{phase}_{k}_loss", True)          # (the LOSS joins the_metric, under mode max)
            if k == "barlowtwins":
                for n in (["img"] if image_view else []) + (["text"] if text_view else []) + \
                        (["both"] if image_view and text_view and not augmentation else []):   # (no `both` attributes under augmentation: the reference raises there)
                    add(f"{k}_loss_invariance_{n}/epoch/{phase}", f"{phase}_{k}_loss_invariance_{n}")
                    add(f"{k}_loss_redundancy_{n}/epoch/{phase}", f"{phase}_{k}_loss_redundancy_{n}",
                        shown=f"{phase}_{k}_loss_redundancy_text" if n == "both" else None)
        else:
            add(f"{k}/{phase}/accuracy_epoch", f"{phase}_{k}_accuracy", True)
            add(f"{k}/{phase}/loss_epoch", f"{phase}_{k}_loss")
        plan.append((k, e))
    return plan


def _epoch_values(pl_module, phase, out):
    """The epoch keys of the reference's wrap-up from ``pl_module.epoch_metrics``, appended to `out`, and ``{phase}/the_metric``.  A slot
    that received nothing gives no key (the reference would log NaN), and the_metric is left out when a slot its sum reads is empty; a
    ``{phase}/the_metric`` the step logs already hold wins."""
    em = pl_module.epoch_metrics
    image_view, text_view, augmentation = _views(pl_module)
    em.reduce_()
    pairs = em.pairs()
    value_of = lambda name: (pairs[name][0] / pairs[name][1]) if name in pairs and pairs[name][1] else None
    the_metric, complete, touched = 0.0, True, []
    if "recalls/ir_r1" in out:
        the_metric += out["recalls/ir_r1"] + out["recalls/tr_r1"]
    for _task, entries in epoch_plan(pl_module.hparams.config["loss_names"], phase, image_view, text_view, augmentation):
        value = 0.0
        for key, attr, shown, is_value in entries:
            v = value_of(shown)
            if v is not None:
                out.setdefault(key, v)
            if attr in em.slots:
                touched.append(em.slots[attr])
            if is_value:
                value = v
        if value is None:
            complete = False
        else:
            the_metric += value
    if touched:
        em.table[torch.tensor(sorted(set(touched)), dtype=torch.int64, device=em.table.device)] = 0.0
    if complete:
        out.setdefault(f"{phase}/the_metric", the_metric)


def epoch_wrapup(pl_module):
    """vilt_utils.epoch_wrapup (:86-313): the per-step values kept in ``pl_module.logged`` pass through and are cleared, the counted
    MLM / MPP accuracies and the recalls follow, and - when ``set_metrics`` has given the module its ``epoch_metrics`` - the reference's
    epoch keys under its names and ``{phase}/the_metric``, its sum of the recalls and every task's value (DESIGN.md "Epoch metrics").
    (As written, the reference's own wrap-up reads undefined ``text_attack`` / ``image_attack`` attributes, :236 - not imitated.)"""
    phase = "train" if pl_module.training else "val"
    out = {k: (float(v) if torch.is_tensor(v) and v.numel() == 1 else v) for k, v in pl_module.logged.items()}
    pl_module.logged = {}
    counts = getattr(pl_module, "mlm_epoch_counts", {}).pop(phase, None)
    if counts is not None:
        # the epoch value of the reference's Accuracy metric: correct / total over every labelled row seen this epoch, then reset
        correct, total = counts.tolist()
        out[f"mlm/{phase}/accuracy_epoch"] = correct / total if total else float("nan")
    counts = getattr(pl_module, "mpp_epoch_counts", {}).pop(phase, None)
    if counts is not None:
        correct, total = counts.tolist()                      # (row, channel) pairs with a label seen this epoch
        out[f"mpp/{phase}/accuracy_epoch"] = correct / total if total else float("nan")
    if pl_module.hparams.config.get("get_recall_metric", False) and not pl_module.training:
        # vilt_utils.py:90-97: image-text retrieval recalls at the end of a validation / test epoch; ir_r1 + tr_r1 joins the_metric.
        # The datasets come from pl_module.irtr_eval_dsets = (text_dset, image_dset) when set, else from the trainer's datamodule
        from . import objectives
        text_dset, image_dset = getattr(pl_module, "irtr_eval_dsets", None) or (None, None)
        rec = objectives.compute_irtr_recall(pl_module, text_dset, image_dset)
        for name, v in zip(("ir_r1", "ir_r5", "ir_r10", "tr_r1", "tr_r5", "tr_r10"), rec):
            out[f"recalls/{name}"] = float(v)
        out["the_metric"] = out.get("the_metric", 0.0) + out["recalls/ir_r1"] + out["recalls/tr_r1"]
    if getattr(pl_module, "epoch_metrics", None) is not None:
        _epoch_values(pl_module, phase, out)
    pl_module.last_epoch_metrics = {"phase": phase, **out}
    return pl_module.last_epoch_metrics


def adamw_segments(specs, total, wd, lr_mult, irtr=False):
    """(segment ends, learning-rate multipliers, weight decays) of the fused AdamW over the arena: one segment per parameter tensor
    (vilt_utils.py:335-393: no decay for biases / LayerNorm, lr x lr_mult for the heads in HEAD_NAMES).  irtr (vilt_module.py:233-239):
    the ITM head is frozen, so row 0 of its weight takes no step and no weight decay (a parameter without a gradient is skipped by
    AdamW); row 1 IS rank_output.weight - not in head_names: base learning rate, decayed.  itm_score.fc.bias needs no split: biases
    are not decayed and bias[0] never receives a gradient (m = v = 0: no step)."""
    ends, mults, wds = [], [], []
    specs = sorted(specs, key=lambda s: s[1])
    for i, (name, off, shape) in enumerate(specs):
        end = specs[i + 1][1] if i + 1 < len(specs) else total
        decay = not any(nd in name for nd in NO_DECAY)
        head = any(bb in name for bb in HEAD_NAMES)
        if irtr and name == "itm_score.fc.weight":
            ends += [off + int(shape[1]), end]
            mults += [0.0, 1.0]
            wds += [0.0, wd]
            continue
        ends.append(end)
        mults.append(lr_mult if head else 1.0)
        wds.append(wd if decay else 0.0)
    return ends, mults, wds


class FusedAdamW:
    """optimizer-like object (``step`` / ``zero_grad`` / ``param_groups`` / ``state_dict``) over the engine's arenas.

    skip_nonfinite / clip_val (config ``skip_nonfinite_steps`` / ``gradient_clip_val``, both off by default): with either set, ``step``
    is the GUARDED step - a statistics pass over the gradient arena takes the decision on the device (rmcl_step_ctl: a non-finite
    gradient drops the step, as the GradScaler of the reference's precision=16 does; clip_val > 0 scales the gradient like
    clip_grad_norm_) and the update kernel reads it there.  No device-to-host copy, no synchronisation: ``t`` counts ATTEMPTED steps on the
    host, the applied / skipped counts live in ``ctl`` and are read by ``counters()`` / ``grad_norm()`` only.  With N > 1 every rank
    sees the same reduced gradient, so every rank takes the same decision without a collective.

    FusedAdam and FusedSGD below are this object with another ``rule``: they replace ``_sweep`` (the update kernel) and nothing else."""

    rule = "adamw"              # recorded by state_dict(); load_state_dict() refuses another rule's state
    has_v = True                # a second-moment arena is kept

    def __init__(self, pl_module, lr, wd, lr_mult, betas=(0.9, 0.98), eps=1e-8, skip_nonfinite=False, clip_val=0.0):
        eng = pl_module.engine
        self.eng = eng
        self.module = pl_module
        self.betas, self.eps = betas, eps
        self.m = torch.zeros_like(eng.q32)
        self.v = torch.zeros_like(eng.q32) if self.has_v else None
        self.t = 0
        ends, mults, wds = adamw_segments(eng.specs, eng.total, wd, lr_mult, eng.irtr)
        dev = eng.device
        self.seg_end = torch.tensor(ends, dtype=torch.int64, device=dev)
        self.seg_mult = torch.tensor(mults, dtype=torch.float32, device=dev)
        self.seg_wd = torch.tensor(wds, dtype=torch.float32, device=dev)
        self.param_groups = [{"lr": lr, "initial_lr": lr}]
        self.grad_scale = 1.0
        self.clip_val = float(clip_val or 0.0)
        self.guarded = bool(skip_nonfinite) or self.clip_val > 0
        if self.guarded:
            self.ctl = torch.zeros(C.sizeof(L.StepCtl), dtype=torch.uint8, device=dev)
            self.stats_ws = torch.zeros(int(lib.rmcl_grad_stats_ws_bytes(I64(eng.q32.numel()))), dtype=torch.uint8, device=dev)

    def zero_grad(self, set_to_none: bool = False):
        self.eng.zero_grads()

    def step(self):
        self.t += 1
        e = self.eng
        self.module.wait_grad_sync()                       # overlapped data-parallel all-reduces (N > 1)
        if self.guarded:
            check(lib.rmcl_grad_stats_f32(P(e.g32), I64(e.q32.numel()), F(self.grad_scale), F(self.clip_val), F(self.betas[0]),
                                          F(self.betas[1]), P(self.stats_ws), P(self.ctl), stream_ptr()), "grad_stats")
        self._sweep()
        e.fold_stale["q"] = True                            # (after a skipped step too: refreshing a shadow that did not move is harmless)
        e.lpT_stale = True
        e.mlm_wt_stale = True

    def _sweep(self):
        """The update kernel over the arenas; guarded, it reads the decision the statistics pass just left in ``ctl``."""
        e = self.eng
        n = I64(e.q32.numel())
        if self.guarded:
            check(lib.rmcl_adamw_guarded_f32(P(e.q32), P(e.g32), P(self.m), P(self.v), P(e.q_lp), P(self.seg_end), P(self.seg_mult),
                                             P(self.seg_wd), int(self.seg_end.numel()), F(self.param_groups[0]["lr"]), F(self.betas[0]),
                                             F(self.betas[1]), F(self.eps), F(self.grad_scale), P(self.ctl), n, stream_ptr()),
                  "adamw_guarded")
        else:
            check(lib.rmcl_adamw_f32(P(e.q32), P(e.g32), P(self.m), P(self.v), P(e.q_lp), P(self.seg_end), P(self.seg_mult),
                                     P(self.seg_wd), int(self.seg_end.numel()), F(self.param_groups[0]["lr"]), F(self.betas[0]),
                                     F(self.betas[1]), F(self.eps), self.t, F(self.grad_scale), n, stream_ptr()),
                  "adamw")

    def read_ctl(self):
        """Host copy of the decision block (synchronises); None on an unguarded optimizer."""
        return L.StepCtl.from_tensor(self.ctl) if self.guarded else None

    def counters(self):
        """(applied, skipped) optimizer steps.  Reads ``ctl``: this call synchronises."""
        if not self.guarded:
            return self.t, 0
        c = self.read_ctl()
        return int(c.applied), int(c.skipped)

    def grad_norm(self):
        """grad_scale * |g| of the last step's FINITE gradient elements, before clipping.  Reads ``ctl``: this call synchronises."""
        if not self.guarded:
            raise RuntimeError("grad_norm(): the gradient statistics run only in the guarded step "
                               "(config skip_nonfinite_steps=True or gradient_clip_val > 0)")
        return float(self.read_ctl().norm)

    def state_dict(self):
        """m, v (where the rule keeps one), the step counts, the rule and the hyper-parameters (tensors, numbers, strings, lists and dicts
        only: torch.load(weights_only=True) reads it).  The segment tables follow from the model and are rebuilt, not stored."""
        applied, skipped = self.counters()
        state = {"m": self.m.detach().cpu()}
        if self.has_v:
            state["v"] = self.v.detach().cpu()
        return {"state": state, "rule": self.rule, "t": int(self.t), "applied": applied, "skipped": skipped,
                "betas": [float(b) for b in self.betas], "eps": float(self.eps), "grad_scale": float(self.grad_scale),
                "param_groups": [dict(g) for g in self.param_groups], "arena_numel": int(self.m.numel())}

    def load_state_dict(self, sd):
        who = type(self).__name__
        rule = sd.get("rule", "adamw")                     # files written before the rule was recorded are AdamW's
        if rule != self.rule:
            raise ValueError(f"{who}.load_state_dict: the checkpoint's optimizer state was written by optim_type={rule!r}, "
                             f"this optimizer is optim_type={self.rule!r}")
        have, want = int(sd["state"]["m"].numel()), int(self.m.numel())
        if have != want or (self.has_v and int(sd["state"]["v"].numel()) != want):
            raise ValueError(f"{who}.load_state_dict: the checkpoint's optimizer state has {have} elements, this model's parameter "
                             f"arena has {want} (another architecture or head set)")
        self.m.copy_(sd["state"]["m"])
        if self.has_v:
            self.v.copy_(sd["state"]["v"])
        self.t = int(sd["t"])
        self.betas, self.eps = tuple(float(b) for b in sd["betas"]), float(sd["eps"])
        self.grad_scale = float(sd["grad_scale"])
        self.param_groups = [dict(g) for g in sd["param_groups"]]
        if self.guarded:
            c = L.StepCtl(applied=int(sd["applied"]), skipped=int(sd["skipped"]), clip_coef=1.0)
            self.ctl.copy_(c.to_tensor(self.ctl.device))
        else:
            self.t = int(sd["applied"])                    # the unguarded kernel's bias corrections follow t: only applied steps count


class FusedAdam(FusedAdamW):
    """``torch.optim.Adam(groups, lr=lr)`` (vilt_utils.py:399-400) over the arenas: betas (0.9, 0.999), eps 1e-8 added AFTER the division
    by sqrt(1 - beta2^t), weight decay coupled into the gradient (include/rmcl.h rmcl_optim_step_f32, RMCL_OPTIM_ADAM)."""

    rule = "adam"
    code = L.OPTIM_ADAM

    def __init__(self, pl_module, lr, wd, lr_mult, betas=(0.9, 0.999), eps=1e-8, skip_nonfinite=False, clip_val=0.0):
        super().__init__(pl_module, lr, wd, lr_mult, betas=betas, eps=eps, skip_nonfinite=skip_nonfinite, clip_val=clip_val)

    def _sweep(self):
        e = self.eng
        check(lib.rmcl_optim_step_f32(self.code, P(e.q32), P(e.g32), P(self.m), P(self.v), P(e.q_lp), P(self.seg_end), P(self.seg_mult),
                                      P(self.seg_wd), int(self.seg_end.numel()), F(self.param_groups[0]["lr"]), F(self.betas[0]),
                                      F(self.betas[1]), F(self.eps), self.t, F(self.grad_scale), P(self.ctl if self.guarded else None),
                                      I64(e.q32.numel()), stream_ptr()), "optim_step")


class FusedSGD(FusedAdam):
    """``torch.optim.SGD(groups, lr=lr, momentum=0.9)`` (vilt_utils.py:401-402): ``m`` is the momentum buffer, there is no ``v`` arena
    (4 bytes of state less per parameter than Adam).  ``betas`` = (momentum, 0) and ``eps`` = 0 keep the surface; the kernel reads only
    betas[0], and the statistics pass of the guarded step writes bias corrections nobody reads."""

    rule = "sgd"
    code = L.OPTIM_SGD
    has_v = False

    def __init__(self, pl_module, lr, wd, lr_mult, momentum=0.9, skip_nonfinite=False, clip_val=0.0):
        super().__init__(pl_module, lr, wd, lr_mult, betas=(momentum, 0.0), eps=0.0, skip_nonfinite=skip_nonfinite, clip_val=clip_val)


OPTIMIZERS = {"adamw": FusedAdamW, "adam": FusedAdam, "sgd": FusedSGD}        # the reference's three optim_type values


class PolySchedule:
    """get_polynomial_decay_schedule_with_warmup as called at vilt_utils.py:423-430; step() per iteration."""

    def __init__(self, opt, warmup, total, end_lr, power):
        self.opt, self.warmup, self.total, self.end_lr, self.power = opt, warmup, total, end_lr, power
        self.base = opt.param_groups[0]["initial_lr"]
        self.n = 0
        self._apply()

    def lr_at(self, step):
        return schedules.poly_lr(step, self.base, self.warmup, self.total, self.end_lr, self.power)

    def _apply(self):
        self.opt.param_groups[0]["lr"] = self.lr_at(self.n)

    def step(self):
        """Once per ATTEMPTED optimizer step: like Lightning's, the schedule also advances on a step the guard dropped."""
        self.n += 1
        self._apply()

    def state_dict(self):
        return {"n": int(self.n), "lr": float(self.opt.param_groups[0]["lr"])}

    def load_state_dict(self, sd):
        self.n = int(sd["n"])
        self._apply()


class CosineSchedule(PolySchedule):
    """get_cosine_schedule_with_warmup (vilt_utils.py:417-421)."""

    def lr_at(self, step):
        return schedules.cosine_lr(step, self.base, self.warmup, self.total)


def set_schedule(pl_module):
    cfg = pl_module.hparams.config
    if cfg["optim_type"] not in OPTIMIZERS:
        raise ValueError(f"set_schedule: optim_type={cfg['optim_type']!r} is none of {sorted(OPTIMIZERS)} (vilt_utils.py:395-402)")
    opt = OPTIMIZERS[cfg["optim_type"]](pl_module, cfg["learning_rate"], cfg["weight_decay"], cfg["lr_mult"],
                                        skip_nonfinite=cfg.get("skip_nonfinite_steps", False), clip_val=cfg.get("gradient_clip_val", 0.0))
    max_steps = cfg["max_steps"]
    if max_steps is None:
        # the reference derives it from the Lightning trainer's dataloader (vilt_utils.py:404-411); rmcl_amd.trainer.Trainer.fit does
        # the same before it calls configure_optimizers(), any other caller states it
        raise ValueError("set_schedule: config['max_steps'] is None - set it to the number of optimizer steps "
                         "(the reference computes it from len(train_dataloader) * max_epoch // accumulate_grad_batches)")
    warmup = cfg["warmup_steps"]
    if isinstance(warmup, float):
        warmup = int(max_steps * warmup)
    if cfg["decay_power"] == "cosine":
        sched = CosineSchedule(opt, warmup, max_steps, cfg["end_lr"], 1)
    else:
        sched = PolySchedule(opt, warmup, max_steps, cfg["end_lr"], cfg["decay_power"])
    return [opt], [{"scheduler": sched, "interval": "step"}]
