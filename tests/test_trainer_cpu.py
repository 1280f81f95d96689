"""CPU: the host arithmetic of rmcl_amd.trainer (the reference's run.py without Lightning) and the resumable-state containers.

  * accumulate_grad_batches = batch_size // (per_gpu_batchsize * num_gpus * num_nodes)              (run.py:80-88)
  * max_steps = len(train_dataloader) * max_epochs // accumulate_grad_batches when the config has None  (vilt_utils.py:404-411)
  * val_check_interval: a float is a fraction of an epoch, an int a number of batches
  * PolySchedule / CosineSchedule state_dict round trip (n, and the lr re-applied)
  * a checkpoint is read by torch.load(weights_only=True) and carries Lightning's key names."""
import os
import random

import pytest
import torch

import rmcl_pkg  # noqa: F401
from rmcl_amd import trainer as T
from rmcl_amd.vilt import config as Cfg
from rmcl_amd.vilt.modules import vilt_utils


def test_new_config_keys_default_to_off():
    cfg = Cfg.default_config()
    assert cfg["skip_nonfinite_steps"] is False and cfg["gradient_clip_val"] == 0.0
    assert Cfg.task_moco()["skip_nonfinite_steps"] is False


@pytest.mark.parametrize("batch_size,per_gpu,gpus,nodes,want", [(4096, 64, 8, 1, 8), (128, 64, 1, 1, 2), (256, 32, [0, 1], 2, 2),
                                                                (128, 48, 1, 1, 2), (64, 64, 1, 1, 1)])
def test_grad_steps_follow_run_py(batch_size, per_gpu, gpus, nodes, want):
    cfg = Cfg.default_config(batch_size=batch_size, per_gpu_batchsize=per_gpu, num_gpus=gpus, num_nodes=nodes)
    n = gpus if isinstance(gpus, int) else len(gpus)
    assert T.grad_steps_of(cfg) == batch_size // (per_gpu * n * nodes) == want


def test_grad_steps_refuse_what_lightning_refuses():
    with pytest.raises(ValueError):
        T.grad_steps_of(Cfg.default_config(batch_size=32, per_gpu_batchsize=64, num_gpus=1, num_nodes=1))      # accumulate_grad_batches = 0
    with pytest.raises(ValueError):
        T.grad_steps_of(Cfg.default_config())                                                                 # per_gpu_batchsize = 0


@pytest.mark.parametrize("n_batches,max_epoch,grad_steps", [(6, 1, 2), (7, 3, 2), (1000, 10, 8), (5, 1, 8)])
def test_max_steps_follow_the_reference(n_batches, max_epoch, grad_steps):
    assert T.derived_max_steps(n_batches, max_epoch, grad_steps) == n_batches * max_epoch // grad_steps


def test_validation_interval():
    assert T.val_check_batches(0.5, 6) == 3 and T.val_check_batches(1.0, 6) == 6 and T.val_check_batches(0.1, 1000) == 100
    assert T.val_check_batches(0.1, 5) == 1                     # never 0 batches
    assert T.val_check_batches(4, 6) == 4
    for bad in (0.0, 1.5, 0, 7, True):
        with pytest.raises(ValueError):
            T.val_check_batches(bad, 6)
    assert [b for b in range(1, 7) if T.should_validate(b, 3)] == [3, 6]
    assert [b for b in range(1, 7) if T.should_validate(b, 4)] == [4]
    # the optimizer steps every grad_steps batches and on the last batch of the epoch
    assert [b for b in range(1, 8) if T.is_last_micro_step(b, 2, 7)] == [2, 4, 6, 7]
    assert [b for b in range(1, 7) if T.is_last_micro_step(b, 2, 6)] == [2, 4, 6]


class _Opt:
    def __init__(self, lr=1e-4):
        self.param_groups = [{"lr": lr, "initial_lr": lr}]


@pytest.mark.parametrize("kind", ["poly", "cosine"])
def test_schedule_state_round_trip(kind):
    make = (lambda o: vilt_utils.PolySchedule(o, 10, 100, 0.0, 1)) if kind == "poly" else (lambda o: vilt_utils.CosineSchedule(o, 10, 100, 0.0, 1))
    a_opt = _Opt()
    a = make(a_opt)
    for _ in range(37):
        a.step()
    sd = a.state_dict()
    assert sd["n"] == 37 and sd["lr"] == a_opt.param_groups[0]["lr"]
    b_opt = _Opt()
    b = make(b_opt)
    assert b_opt.param_groups[0]["lr"] == 0.0                   # warm-up, n = 0
    b.load_state_dict(sd)
    assert b.n == 37 and b_opt.param_groups[0]["lr"] == a_opt.param_groups[0]["lr"] == a.lr_at(37)   # _apply() ran after the load
    a.step()
    b.step()
    assert b_opt.param_groups[0]["lr"] == a_opt.param_groups[0]["lr"]


class _Model:
    """What save_checkpoint reads of a module, on the CPU."""

    def __init__(self):
        self.w = {"a.weight": torch.arange(6.0).reshape(2, 3), "proj_queue_ptr": torch.tensor([5])}

    def state_dict(self):
        return self.w

    def training_state(self):
        v, internal, gauss = random.getstate()
        return {"pass_counter": 7, "seed_base": 1, "queue_ptr": 5, "logged": {"moco/train/loss": torch.tensor(2.5), "n": 3},
                "torch_rng": torch.get_rng_state(), "python_rng": [v, list(internal), gauss]}


class _OptState(_Opt):
    t = 4

    def state_dict(self):
        return {"state": {"m": torch.ones(8), "v": torch.full((8,), 2.0)}, "t": 4, "applied": 3, "skipped": 1, "betas": [0.9, 0.98], "eps": 1e-8,
                "grad_scale": 0.5, "param_groups": [dict(g) for g in self.param_groups], "arena_numel": 8}


def test_checkpoint_loads_with_weights_only_and_has_lightnings_keys(tmp_path):
    opt = _OptState()
    sched = vilt_utils.PolySchedule(opt, 2, 10, 0.0, 1)
    sched.step()
    path = str(tmp_path / "sub" / "last.ckpt")
    random.seed(3)
    assert T.save_checkpoint(path, _Model(), opt, sched, global_step=4, epoch=1, batches_in_epoch=2, best_metric=0.25) == path
    assert os.listdir(tmp_path / "sub") == ["last.ckpt"]        # the temporary name is gone
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"state_dict", "optimizer_states", "lr_schedulers", "global_step", "epoch", "training_state", "batches_in_epoch", "best_metric"}
    assert (ck["global_step"], ck["epoch"], ck["batches_in_epoch"], ck["best_metric"]) == (4, 1, 2, 0.25)
    assert torch.equal(ck["state_dict"]["a.weight"], torch.arange(6.0).reshape(2, 3))
    o = ck["optimizer_states"][0]
    assert (o["t"], o["applied"], o["skipped"], o["arena_numel"]) == (4, 3, 1, 8) and torch.equal(o["state"]["v"], torch.full((8,), 2.0))
    assert ck["lr_schedulers"][0]["n"] == 1
    ts = ck["training_state"]
    assert ts["pass_counter"] == 7 and ts["logged"]["n"] == 3 and float(ts["logged"]["moco/train/loss"]) == 2.5
    version, internal, gauss = ts["python_rng"]
    want = random.random()
    random.setstate((version, tuple(internal), gauss))          # Python's generator continues from the file
    assert random.random() == want


def test_to_device_moves_tensors_and_lists_of_tensors():
    b = T.to_device({"image": [torch.zeros(1)], "text_ids": torch.ones(2), "text": ["a"], "qid": [3]}, "cpu")
    assert torch.is_tensor(b["image"][0]) and b["text"] == ["a"] and b["qid"] == [3]
