"""The reference's ``run.py`` without Lightning: gradient accumulation, the stopping rule, periodic validation, last / best checkpoints,
resume and the ``test_only`` switch around ``ViLTransformerSS.training_step`` and the fused optimizer.

    trainer = Trainer(config)
    trainer.fit(model, train_loader, val_loader)       # or trainer.run(model, train_loader, val_loader, test_loader)
    trainer.run(model)                                 # no loaders: MTDataModule(config) builds them from config["data_root"]

What it takes from ``run.py``: ``accumulate_grad_batches`` (:86-88, :105), ``max_steps`` / ``max_epochs`` (:90-100), ``val_check_interval``
(:111), a ModelCheckpoint with ``save_last`` and ``save_top_k=1`` on ``val/the_metric``, mode max (:46-52), ``resume_from_checkpoint`` (:108),
``fast_dev_run`` (:110) and ``test_only`` (:114-118).  ``precision=16`` has no scaler here (the engine computes in bf16 / fp32); the part of it
that matters to a long run - a step with a non-finite gradient is dropped - is ``config["skip_nonfinite_steps"]`` (FusedAdamW's guarded step).
No logger: ``model.logged`` and ``model.last_epoch_metrics`` are the log.

A checkpoint is ONE file under Lightning's key names (``state_dict``, ``optimizer_states``, ``lr_schedulers``, ``global_step``, ``epoch``) plus
``training_state`` (ViLTransformerSS.training_state) and ``batches_in_epoch``; it holds tensors, numbers, strings, lists and dicts only, so
``torch.load(weights_only=True)`` reads it, and ``config["load_path"]`` on it loads the weights like a reference checkpoint."""
from __future__ import annotations

import itertools
import os
import random

import torch

LAST, BEST = "last.ckpt", "best.ckpt"
MONITOR = "val/the_metric"


def seed_everything(seed: int):
    """pl.seed_everything (run.py:38): Python, numpy and torch."""
    random.seed(seed)
    try:
        import numpy as np
        np.random.seed(seed)
    except ImportError:
        pass
    torch.manual_seed(seed)


def grad_steps_of(config) -> int:
    """accumulate_grad_batches of run.py:80-88."""
    num_gpus = config["num_gpus"] if isinstance(config["num_gpus"], int) else len(config["num_gpus"])
    per_step = config["per_gpu_batchsize"] * num_gpus * config["num_nodes"]
    if per_step <= 0:
        raise ValueError("per_gpu_batchsize * num_gpus * num_nodes must be positive (config['per_gpu_batchsize'] defaults to 0: set it)")
    steps = config["batch_size"] // per_step
    if steps < 1:
        raise ValueError(f"batch_size {config['batch_size']} is smaller than one step of all devices ({per_step}): Lightning refuses "
                         "accumulate_grad_batches = 0")
    return steps


def derived_max_steps(n_batches: int, max_epoch: int, grad_steps: int) -> int:
    """max_steps when the config leaves it None (vilt_utils.py:404-411)."""
    return n_batches * max_epoch // grad_steps


def val_check_batches(interval, n_batches: int) -> int:
    """Validate after every this many training batches.  A float is a fraction of the epoch, an int a number of batches (Lightning's
    val_check_interval, run.py:111)."""
    if isinstance(interval, bool):
        raise ValueError("val_check_interval must be a float in (0, 1] or an int")
    if isinstance(interval, int):
        if interval < 1 or interval > n_batches:
            raise ValueError(f"val_check_interval = {interval} batches, but an epoch has {n_batches}")
        return interval
    if not 0.0 < interval <= 1.0:
        raise ValueError(f"val_check_interval = {interval}: a float must lie in (0, 1]")
    return max(1, int(n_batches * interval))


def should_validate(batches_done: int, every: int) -> bool:
    return batches_done % every == 0


def is_last_micro_step(batches_done: int, grad_steps: int, n_batches: int) -> bool:
    """The optimizer steps after every grad_steps batches and, like Lightning, on the last batch of an epoch."""
    return batches_done % grad_steps == 0 or batches_done == n_batches


def to_device(batch, device):
    def mv(v):
        if torch.is_tensor(v):
            return v.to(device)
        if isinstance(v, list) and v and torch.is_tensor(v[0]):
            return [t.to(device) for t in v]
        return v
    return {k: mv(v) for k, v in batch.items()}


def save_checkpoint(path, model, opt, sched, **progress):
    """progress: global_step, epoch, batches_in_epoch and anything else made of tensors, numbers, strings, lists and dicts.  Written to a
    temporary name in the same directory and renamed, so a reader never sees half a file."""
    ckpt = {"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
            "optimizer_states": [opt.state_dict()],
            "lr_schedulers": [sched.state_dict()],
            "global_step": int(progress.pop("global_step", opt.t)),
            "epoch": int(progress.pop("epoch", 0)),
            "batches_in_epoch": int(progress.pop("batches_in_epoch", 0)),
            "training_state": model.training_state()}
    ckpt.update(progress)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)
    return path


def load_checkpoint(path, model, opt, sched):
    """Restores model, optimizer, schedule and training state; returns the file's dict (global_step, epoch, batches_in_epoch, ...).  The
    optimizer's arena size is checked before anything is written."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    have, want = int(ckpt["optimizer_states"][0]["arena_numel"]), int(opt.m.numel())
    if have != want:
        raise ValueError(f"{path}: written by a model whose parameter arena has {have} elements, this model's has {want}")
    model.load_state_dict(ckpt["state_dict"], strict=True)
    opt.load_state_dict(ckpt["optimizer_states"][0])
    sched.load_state_dict(ckpt["lr_schedulers"][0])
    model.load_training_state(ckpt["training_state"])
    return ckpt


class Trainer:
    def __init__(self, config, ckpt_dir=None):
        self.config = config
        self.grad_steps = grad_steps_of(config)
        self.ckpt_dir = ckpt_dir or os.path.join(config.get("log_dir", "result"), str(config.get("exp_name", "vilt")), "checkpoints")
        self.global_step = 0
        self.epoch = 0
        self.batches_in_epoch = 0
        self.best_metric = None
        self.validations = 0
        self.optimizer = self.scheduler = None
        self.datamodule = None

    def attach_datamodule(self, model):
        """run.py:40 for the calls that bring no loader: ``MTDataModule(config, dist=<a process group is initialised>)``, set up once and
        kept as ``self.datamodule``.  ``model.trainer = self`` is what ``compute_irtr_recall`` (get_recall_metric) reads its validation
        datasets through; a VQA datamodule hands the model its ``id2answer``."""
        if self.datamodule is None:
            from .vilt.datamodules import MTDataModule
            dist = torch.distributed.is_available() and torch.distributed.is_initialized()
            self.datamodule = MTDataModule(self.config, dist=dist)
            self.datamodule.setup("fit")
        model.trainer = self
        vqa = self.datamodule.dm_dicts.get("vqa")
        if vqa is not None:
            model.id2answer = vqa.id2answer
        return self.datamodule

    # run.py:114-118
    def run(self, model, train_loader=None, val_loader=None, test_loader=None):
        if self.config.get("test_only", False):
            return self.test(model, test_loader if test_loader is not None else val_loader)
        return self.fit(model, train_loader, val_loader)

    def _metrics(self, model):
        """vilt_module.py:253 calls set_metrics in every model's constructor; here the trainer does, once, unless config["epoch_metrics"]
        is false - a model stepped without a trainer launches nothing for metrics"""
        if getattr(model, "epoch_metrics", None) is None and self.config.get("epoch_metrics", True):
            from .vilt.modules import vilt_utils
            vilt_utils.set_metrics(model)

    def _eval_loop(self, model, loader, step, end):
        self._metrics(model)
        was_training = model.training
        model.eval()
        with torch.no_grad():
            for i, batch in enumerate(loader):
                step(to_device(batch, model.device), i)
                if self.config.get("fast_dev_run", False):
                    break
        end()
        model.train(was_training)
        return getattr(model, "last_epoch_metrics", {})

    def test(self, model, loader=None):
        if loader is None:                                   # no loader: the config's datamodule (config["datasets"], config["data_root"])
            loader = self.attach_datamodule(model).test_dataloader()
        return self._eval_loop(model, loader, model.test_step, model.test_epoch_end)

    def validate(self, model, loader):
        self.validations += 1
        return self._eval_loop(model, loader, model.validation_step, model.validation_epoch_end)

    def _save(self, name, model, n_batches):
        epoch, done = (self.epoch + 1, 0) if self.batches_in_epoch == n_batches else (self.epoch, self.batches_in_epoch)
        progress = dict(global_step=self.global_step, epoch=epoch, batches_in_epoch=done, validations=self.validations)
        if self.best_metric is not None:
            progress["best_metric"] = float(self.best_metric)
        if done % self.grad_steps != 0:                     # mid-accumulation: the gradient arena is part of the state
            progress["grad_accum"] = model.engine.g32.detach().cpu()
        return save_checkpoint(os.path.join(self.ckpt_dir, name), model, self.optimizer, self.scheduler, **progress)

    def _after_validation(self, model, metrics, n_batches):
        value = metrics.get(MONITOR, metrics.get("the_metric"))
        if value is not None and (self.best_metric is None or float(value) > self.best_metric):   # mode max, save_top_k = 1
            self.best_metric = float(value)
            self._save(BEST, model, n_batches)
        self._save(LAST, model, n_batches)

    def fit(self, model, train_loader=None, val_loader=None):
        cfg = self.config
        if cfg.get("test_only", False):
            return self.test(model, val_loader)
        if train_loader is None:                             # no loader: the config's datamodule, its validation loader included
            dm = self.attach_datamodule(model)
            train_loader = dm.train_dataloader()
            val_loader = dm.val_dataloader() if val_loader is None else val_loader
        self._metrics(model)
        fast = bool(cfg.get("fast_dev_run", False))
        n_batches = len(train_loader)
        max_epochs = 1000                                    # run.py:99
        if cfg["max_steps"] is None:
            max_epochs = cfg["max_epoch"]
            cfg["max_steps"] = derived_max_steps(n_batches, cfg["max_epoch"], self.grad_steps)
        model.hparams.config["max_steps"] = cfg["max_steps"]
        max_steps = cfg["max_steps"]
        (opt,), (sd,) = model.configure_optimizers()
        sched = sd["scheduler"]
        opt.grad_scale = 1.0 / self.grad_steps
        self.optimizer, self.scheduler = opt, sched
        every = val_check_batches(cfg.get("val_check_interval", 1.0), n_batches) if val_loader is not None else 0
        if cfg.get("resume_from"):
            ck = load_checkpoint(cfg["resume_from"], model, opt, sched)
            self.global_step, self.epoch, self.batches_in_epoch = ck["global_step"], ck["epoch"], ck["batches_in_epoch"]
            self.best_metric = ck.get("best_metric")
            self.validations = ck.get("validations", 0)
            if "grad_accum" in ck:
                model.engine.g32.copy_(ck["grad_accum"])
        model.train()
        sampler = getattr(train_loader, "sampler", None)
        while self.epoch < max_epochs and self.global_step < max_steps:
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(self.epoch)
            stop = False
            for batch_idx, batch in itertools.islice(enumerate(train_loader), self.batches_in_epoch, None):
                last = is_last_micro_step(batch_idx + 1, self.grad_steps, n_batches) or fast
                model.sync_grads = last
                loss = model.training_step(to_device(batch, model.device), batch_idx)
                loss.backward()
                if last:
                    opt.step()
                    sched.step()
                    opt.zero_grad()
                    self.global_step += 1
                self.batches_in_epoch = batch_idx + 1
                if fast:
                    if val_loader is not None:
                        self.validate(model, val_loader)
                    return self
                if every and should_validate(self.batches_in_epoch, every):
                    self._after_validation(model, self.validate(model, val_loader), n_batches)
                if self.global_step >= max_steps:
                    stop = True
                    break
            if stop:
                break
            model.training_epoch_end()
            self.epoch += 1
            self.batches_in_epoch = 0
        model.sync_grads = True
        return self
