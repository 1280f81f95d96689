"""-m gpu: the guarded optimizer step inside a training step, resumable state and rmcl_amd.trainer on the smallest module (2 layers, B = 4,
queue 1024, vocabulary 2048, task_moco with PGD K = 1).

Round trip     save after 2 steps with dropout on, load into FRESH objects (built from another seed): every tensor of state_dict(), m and v
               bit-equal; t, the counters, the schedule, pass_counter and queue_ptr equal; the next pass draws the same dropout seed.
Continuation   runs A (4 steps), A' (the same again) and B (2 steps, save, fresh objects, load, 2 steps).  The MoCo step is NOT
               bit-reproducible run to run (float atomics of the cls-row scatter, tests/test_path_gpu.py
               test_half_batch_lanes_give_the_one_chain_step), so B is held to that test's rule: its relative distance from A is at most
               max(1e-5, 10 * distance(A, A')), for the parameter arena and for the losses of steps 3 and 4.
Guard          an inf written into the gradient arena after backward(): the step changes nothing, the counters and the schedule move,
               opt.step() runs with torch's synchronisation check armed.
Trainer        6 batches, grad_steps = 2: accumulation, validation interval, last / best checkpoints, resume, test_only."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L  # noqa: E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd import trainer as T  # noqa: E402
from rmcl_amd.vilt.config import task_moco  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402

SMALL = dict(num_layers=2, num_negative=1024, per_gpu_batchsize=4, adv_steps_img=1, vocab_size=2048)
OCFG = O.default_config(**SMALL)


def config(**over):
    cfg = task_moco(**SMALL, drop_rate=0.1, image_view=True, text_view=False, num_gpus=1, num_nodes=1, batch_size=4, learning_rate=2e-4,
                    warmup_steps=1, max_steps=10)
    cfg.update(over)
    return cfg


def dev_batch(batch):
    return T.to_device(batch, DEV)


def build(cfg, seed=0, dtype="bf16"):
    T.seed_everything(seed)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype=dtype)
    m.train()
    (opt,), (sd,) = m.configure_optimizers()
    return m, opt, sd["scheduler"]


def train_steps(m, opt, sched, steps):
    """steps: indices; step i trains on synthetic batch i.  Returns the losses."""
    losses = []
    for i in steps:
        loss = m.training_step(dev_batch(O.synthetic_batch(OCFG, 4, 100 + i)), i)
        loss.backward()
        opt.step()
        sched.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    return losses


def rel(a, b):
    return float((a.double() - b.double()).norm() / a.double().norm())


# ------------------------------------------------------------------------------------------ round trip
def test_round_trip_restores_every_piece_of_state(tmp_path):
    cfg = config(skip_nonfinite_steps=True)
    m, opt, sched = build(cfg, seed=0)
    train_steps(m, opt, sched, [0, 1])
    path = str(tmp_path / "two.ckpt")
    T.save_checkpoint(path, m, opt, sched, global_step=2, epoch=0, batches_in_epoch=2)
    assert set(torch.load(path, map_location="cpu", weights_only=True)) >= {"state_dict", "optimizer_states", "lr_schedulers", "global_step",
                                                                              "epoch", "training_state", "batches_in_epoch"}
    m2, opt2, sched2 = build(cfg, seed=77)                                       # other weights, another queue
    assert not torch.equal(m2.engine.q32, m.engine.q32)
    ck = T.load_checkpoint(path, m2, opt2, sched2)
    assert (ck["global_step"], ck["epoch"], ck["batches_in_epoch"]) == (2, 0, 2)
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert set(sd) == set(sd2) and {"proj_queue", "proj_queue_ptr"} <= set(sd)
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    assert torch.equal(m2.engine.q32, m.engine.q32) and torch.equal(m2.engine.k32, m.engine.k32)
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and float(opt.v.abs().max()) > 0
    assert opt2.t == opt.t == 2 and opt2.counters() == opt.counters() == (2, 0)
    assert opt2.betas == opt.betas and opt2.eps == opt.eps and opt2.grad_scale == opt.grad_scale
    assert sched2.n == sched.n == 2 and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] > 0
    assert m2.engine.pass_counter == m.engine.pass_counter > 0 and m2.engine.seed_base == m.engine.seed_base
    assert m2.queue_ptr == m.queue_ptr == 8
    # the next pass draws the same dropout seed: every encoder pass of one more step, logged by the engine
    batch = dev_batch(O.synthetic_batch(OCFG, 4, 102))
    logs = []
    for mod in (m, m2):
        mod.engine.pass_log = []
        mod.training_step(batch, 2).backward()
        logs.append([(e["seed"], e["p"], e["mode"], e["key"]) for e in mod.engine.pass_log])
        mod.engine.pass_log = None
    assert logs[0] == logs[1] and len(logs[0]) >= 3 and any(p > 0 for _, p, _, _ in logs[0])

    # config["load_path"] on the same file loads the weights, as it loads a reference checkpoint
    m3 = ViLTransformerSS(config(load_path=path), device=DEV, compute_dtype="bf16")
    assert m3.load_report["missing"] == [] and m3.load_report["unexpected"] == []
    file_sd = ck["state_dict"]
    for k, v in m3.state_dict().items():
        assert torch.equal(v.cpu(), file_sd[k]), k

    # a model with another arena refuses the file and names both sizes
    m4, opt4, sched4 = build(config(num_layers=1), seed=0)
    before = m4.engine.q32.clone()
    with pytest.raises(ValueError) as err:
        T.load_checkpoint(path, m4, opt4, sched4)
    assert str(opt.m.numel()) in str(err.value) and str(opt4.m.numel()) in str(err.value) and opt.m.numel() != opt4.m.numel()
    with pytest.raises(ValueError) as err:
        opt4.load_state_dict(ck["optimizer_states"][0])
    assert str(opt.m.numel()) in str(err.value) and str(opt4.m.numel()) in str(err.value)
    assert torch.equal(m4.engine.q32, before) and opt4.t == 0


# ------------------------------------------------------------------------------------------ continuation
def test_a_resumed_run_continues_like_the_uninterrupted_one(tmp_path):
    """The learning rate (1e-6, no warm-up) is chosen for the rule's floor.  The run-to-run noise of a LOSS is one number: were it far
    above 1e-5, |A - B| and |A - A'| would be two draws of one distribution and their ratio would pass 10 about one time in sixteen
    (P(|Cauchy| > 10)).  A step's own noise is ~1e-7 relative; what the earlier steps' parameter noise adds grows with the learning rate
    (at 2e-4 this recipe measured 5e-6 ... 4e-4 on steps 3 and 4), so at 1e-6 both stay under the floor and the loss checks do not
    flicker.  What a broken resume does is far above it: other dropout seeds move the loss by > 1e-3 relative, lost moments change a
    step's update by about lr per element against weights of ~0.02 - 5e-5 of the arena."""
    cfg = config(skip_nonfinite_steps=True, gradient_clip_val=5.0, learning_rate=1e-6, warmup_steps=0)

    def straight():
        m, opt, sched = build(cfg, seed=0)
        losses = train_steps(m, opt, sched, range(4))
        return m.engine.q32.clone(), losses, opt.counters()

    a, a2 = straight(), straight()
    m, opt, sched = build(cfg, seed=0)
    first = train_steps(m, opt, sched, range(2))
    path = str(tmp_path / "mid.ckpt")
    T.save_checkpoint(path, m, opt, sched, global_step=2, epoch=0, batches_in_epoch=2)
    del m, opt, sched
    m, opt, sched = build(cfg, seed=5)                                           # fresh objects, nothing in common but the file
    T.load_checkpoint(path, m, opt, sched)
    later = train_steps(m, opt, sched, range(2, 4))
    b = (m.engine.q32.clone(), first + later, opt.counters())
    assert a[2] == a2[2] == b[2] == (4, 0)
    noise, dist = rel(a[0], a2[0]), rel(a[0], b[0])
    lnoise = [abs(x - y) / abs(x) for x, y in zip(a[1], a2[1])]
    ldist = [abs(x - y) / abs(x) for x, y in zip(a[1], b[1])]
    bit_equal = torch.equal(a[0], a2[0]) and torch.equal(a[0], b[0]) and a[1] == a2[1] == b[1]
    print(f"resume: arena |A - A'| / |A| = {noise:.3e}, |A - B| / |A| = {dist:.3e}; losses A {a[1]} A' {a2[1]} B {b[1]}; "
          f"the three runs {'ARE' if bit_equal else 'are NOT'} bit-equal")
    assert dist <= max(1e-5, 10 * noise), (dist, noise)
    for i in (2, 3):                                                             # steps 3 and 4: the ones taken after the load
        assert ldist[i] <= max(1e-5, 10 * lnoise[i]), (i, ldist[i], lnoise[i])
    assert ldist[0] <= max(1e-5, 10 * lnoise[0]) and ldist[1] <= max(1e-5, 10 * lnoise[1])


# ------------------------------------------------------------------------------------------ the guard in a step
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_nonfinite_gradient_drops_the_step_without_a_host_round_trip(dtype):
    cfg = config(skip_nonfinite_steps=True)
    m, opt, sched = build(cfg, seed=0, dtype=dtype)
    e = m.engine
    assert opt.guarded
    train_steps(m, opt, sched, [0])                                              # one clean step: m and v are not zero
    assert opt.counters() == (1, 0) and opt.grad_norm() > 0
    loss = m.training_step(dev_batch(O.synthetic_batch(OCFG, 4, 101)), 1)
    loss.backward()
    e.g32[12345] = float("inf")
    torch.cuda.synchronize()
    keep = [t.clone() for t in (e.q32, opt.m, opt.v)] + ([e.q_lp.clone()] if e.q_lp is not None else [])
    lr_before = opt.param_groups[0]["lr"]
    has_mode = hasattr(torch.cuda, "set_sync_debug_mode")
    if has_mode:
        torch.cuda.set_sync_debug_mode("error")                                  # any synchronising call inside step() now raises
    try:
        opt.step()
    finally:
        if has_mode:
            torch.cuda.set_sync_debug_mode("default")
    sched.step()
    opt.zero_grad()
    now = [e.q32, opt.m, opt.v] + ([e.q_lp] if e.q_lp is not None else [])
    for a, b in zip(now, keep):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert opt.counters() == (1, 1) and opt.t == 2
    c = opt.read_ctl()
    assert c.skip == 1 and c.nonfinite == 1
    assert sched.n == 2 and opt.param_groups[0]["lr"] != lr_before               # the schedule steps on a dropped step too
    train_steps(m, opt, sched, [2])                                              # the next clean step moves the weights
    assert opt.counters() == (2, 1) and opt.t == 3
    assert not torch.equal(e.q32, keep[0]) and torch.isfinite(e.q32).all()
    c = opt.read_ctl()
    assert c.skip == 0 and c.nonfinite == 0 and c.bc1 == float(torch.tensor(1.0 - float(torch.tensor(0.9)) ** 2, dtype=torch.float32))
    if e.q_lp is not None:
        assert torch.equal(e.q_lp[:4096].float(), e.q32[:4096].to(torch.bfloat16).float())


def test_default_config_keeps_the_unguarded_step():
    m, opt, sched = build(config(), seed=0)
    assert not opt.guarded and not hasattr(opt, "ctl")
    train_steps(m, opt, sched, [0])
    assert opt.counters() == (1, 0)
    with pytest.raises(RuntimeError):
        opt.grad_norm()


# ------------------------------------------------------------------------------------------ two ranks
def test_two_ranks_take_the_same_decision_without_a_collective():
    """tools/guarded_two_rank.py: two processes on cuda:0 over gloo (tests/gpu_util.py has no rehearsal of its own; this is the launch
    tests/test_mpp_gpu.py uses).  The last rank's LOCAL gradient is poisoned before the reduction of an accumulated step: both ranks drop
    that step, neither writes a byte, and after one more clean step their parameters and moments hold the same bits."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29743", os.path.join(root, "tools", "guarded_two_rank.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    print(rec)
    assert rec["world_size"] == 2
    assert rec["counters_after_skip"] == [[1, 1], [1, 1]] and rec["counters_final"] == [[2, 1], [2, 1]]
    assert rec["skipped_step_wrote_nothing"] == [True, True] and rec["clean_step_moved_the_weights"] == [True, True]
    assert rec["ranks_bit_identical"] is True and rec["finite"] is True


# ------------------------------------------------------------------------------------------ trainer
def loaders():
    return [O.synthetic_batch(OCFG, 4, 200 + i) for i in range(6)], [O.synthetic_batch(OCFG, 4, 300)]


def spy(model, metrics=None):
    """Records sync_grads at every training micro-step; logs the next injected val/the_metric at every validation step."""
    seen = {"sync": [], "val": 0, "test": 0}
    train, val, test = model.training_step, model.validation_step, model.test_step

    def training_step(batch, i):
        seen["sync"].append(bool(model.sync_grads))
        return train(batch, i)

    def validation_step(batch, i):
        out = val(batch, i)
        if metrics:
            model.log(T.MONITOR, metrics[min(seen["val"], len(metrics) - 1)])
        seen["val"] += 1
        return out

    def test_step(batch, i):
        seen["test"] += 1
        return test(batch, i)

    model.training_step, model.validation_step, model.test_step = training_step, validation_step, test_step
    return seen


def test_trainer_accumulates_validates_checkpoints_and_resumes(tmp_path):
    train, val = loaders()
    over = dict(batch_size=8, max_steps=None, max_epoch=1, warmup_steps=1, skip_nonfinite_steps=True)
    cfg = config(val_check_interval=0.5, **over)
    T.seed_everything(0)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype="bf16")
    seen = spy(m, metrics=[0.7, 0.3])
    tr = T.Trainer(cfg, ckpt_dir=str(tmp_path / "a"))
    assert tr.grad_steps == 2
    tr.fit(m, train, val)
    assert cfg["max_steps"] == 3                                                 # 6 batches * 1 epoch // 2, set before configure_optimizers
    assert tr.global_step == 3 and tr.optimizer.t == 3 and tr.optimizer.counters() == (3, 0) and tr.scheduler.n == 3
    assert tr.optimizer.grad_scale == 0.5
    assert seen["sync"] == [False, True] * 3                                     # no reduction on the odd micro-steps
    assert tr.validations == 2 and seen["val"] == 2
    last = torch.load(str(tmp_path / "a" / T.LAST), map_location="cpu", weights_only=True)
    best = torch.load(str(tmp_path / "a" / T.BEST), map_location="cpu", weights_only=True)
    assert (last["global_step"], last["epoch"], last["batches_in_epoch"]) == (3, 1, 0)
    assert (best["global_step"], best["epoch"], best["batches_in_epoch"], best["best_metric"]) == (1, 0, 3, 0.7)   # 0.3 did not replace it
    assert "grad_accum" in best and "grad_accum" not in last                    # batch 3 of 6 is mid-accumulation
    assert tr.best_metric == 0.7 and m.training and m.sync_grads
    straight = (tr.global_step, tr.scheduler.n, tr.optimizer.param_groups[0]["lr"])

    # a checkpoint at optimizer step 2 (validation after 4 batches), then a fresh trainer resumes from it
    cfg_b = config(val_check_interval=4, **over)
    T.seed_everything(0)
    mb = ViLTransformerSS(cfg_b, device=DEV, compute_dtype="bf16")
    spy(mb, metrics=[0.1])
    T.Trainer(cfg_b, ckpt_dir=str(tmp_path / "b")).fit(mb, train, val)
    mid = str(tmp_path / "b" / T.BEST)                                           # (last.ckpt was written by the same validation)
    ck = torch.load(mid, map_location="cpu", weights_only=True)
    assert (ck["global_step"], ck["epoch"], ck["batches_in_epoch"]) == (2, 0, 4)
    cfg_c = config(val_check_interval=0.5, resume_from=mid, **over)
    T.seed_everything(9)
    mc = ViLTransformerSS(cfg_c, device=DEV, compute_dtype="bf16")
    seen_c = spy(mc, metrics=[0.05])
    tc = T.Trainer(cfg_c, ckpt_dir=str(tmp_path / "c"))
    tc.fit(mc, train, val)
    assert seen_c["sync"] == [False, True]                                       # only batches 5 and 6 were trained
    assert (tc.global_step, tc.scheduler.n, tc.optimizer.param_groups[0]["lr"]) == straight
    assert tc.optimizer.t == 3 and tc.optimizer.counters() == (3, 0)
    assert tc.best_metric == 0.1 and not os.path.exists(str(tmp_path / "c" / T.BEST))   # 0.05 is no improvement on the resumed 0.1
    assert os.path.exists(str(tmp_path / "c" / T.LAST))


def test_trainer_test_only_and_fast_dev_run(tmp_path):
    train, val = loaders()
    cfg = config(test_only=True, batch_size=8)
    T.seed_everything(0)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype="bf16")
    seen = spy(m)
    q0 = m.engine.q32.clone()
    tr = T.Trainer(cfg, ckpt_dir=str(tmp_path / "t"))
    metrics = tr.run(m, train, val, test_loader=train[:2])
    assert seen["sync"] == [] and seen["test"] == 2 and seen["val"] == 2         # (test_step goes through validation_step)
    assert metrics["phase"] == "val" and torch.equal(m.engine.q32, q0) and tr.global_step == 0
    assert not os.path.exists(str(tmp_path / "t"))
    cfg = config(fast_dev_run=True, batch_size=8)
    T.seed_everything(0)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype="bf16")
    seen = spy(m)
    tr = T.Trainer(cfg, ckpt_dir=str(tmp_path / "f")).fit(m, train, val)
    assert len(seen["sync"]) == 1 and seen["val"] == 1 and tr.global_step == 1
