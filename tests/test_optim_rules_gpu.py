"""-m gpu: optim_type "adam" and "sgd" (FusedAdam, FusedSGD of vilt/modules/vilt_utils.py) on the smallest module of
tests/test_resume_gpu.py (2 layers, B = 4, queue 1024, vocabulary 2048).

Parity        three optimizer steps on seeded gradients written straight into the gradient arena (no backward: only the optimizer is
              under test), every trained parameter against torch.optim.Adam / torch.optim.SGD(momentum=0.9) in float64 on the CPU over
              copies grouped by the reference's name rules (vilt_utils.py:335-393, restated here).  Bound per parameter, the kernel
              test's rule: |got - fp64| <= 4 * max(e32, 2^-23 * max|fp64|), e32 = the deviation of the SAME torch optimizer run in
              float32.  The learning rate is a power of two so that lr and lr * lr_mult are the same numbers in fp32 and float64.
IRTR          row 0 of itm_score.fc.weight (lr_mult = 0) keeps its bits under a gradient that is not zero there; row 1 moves.
Round trip    steps, checkpoint (torch.load(weights_only=True) reads it), fresh model and optimizer, one more step on the same gradient:
              bit-equal parameters and state.  The SGD state holds no v.
Compatibility another rule's state is refused with a ValueError naming both; a state dict without a rule entry is AdamW's.
Guard         a NaN in the gradient drops the step under both rules.
Trainer       optim_type="sgd" through Trainer.fit: accumulation, checkpoint, resume; the resumed run against the uninterrupted one by the
              run-to-run rule of test_a_resumed_run_continues_like_the_uninterrupted_one.
Default       optim_type="adamw" builds a FusedAdamW whose unguarded step is one rmcl_adamw_f32 call."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV  # noqa: E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd import trainer as T  # noqa: E402
from rmcl_amd.vilt.config import task_finetune_irtr_coco, task_moco  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, vilt_utils  # noqa: E402

SMALL = dict(num_layers=2, num_negative=1024, per_gpu_batchsize=4, adv_steps_img=1, vocab_size=2048)
OCFG = O.default_config(**SMALL)
FACTOR = 4.0                                 # tests/test_step_kernels_gpu.py ADAMW_FACTOR
LR, LR_MULT, WD = 2.0 ** -12, 10, 0.01
RULES = ["adam", "sgd"]
# vilt_utils.py:335-346 of the reference, restated
no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight", "norm.bias", "norm.weight", "norm1.bias", "norm1.weight", "norm2.bias", "norm2.weight"]
head_names = ["vqa_classifier", "nlvr2_classifier", "moco_head", "barlowtwinshead"]


def config(**over):
    cfg = task_moco(**SMALL, drop_rate=0.1, image_view=True, text_view=False, num_gpus=1, num_nodes=1, batch_size=4, learning_rate=LR,
                    lr_mult=LR_MULT, weight_decay=WD, warmup_steps=0, max_steps=10)
    cfg.update(over)
    return cfg


def build(cfg, seed=0, dtype="bf16"):
    T.seed_everything(seed)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype=dtype)
    m.train()
    (opt,), (sd,) = m.configure_optimizers()
    return m, opt, sd["scheduler"]


def seeded_grad(m, seed, scale=1e-3):
    """A seeded gradient in every slot of the gradient arena that a trained parameter owns; zero elsewhere, as a backward leaves the
    slots nobody owns (padding, heads of other tasks) - state_dict() does not carry those."""
    eng = m.engine
    if not hasattr(eng, "_owned"):
        eng.g32.zero_()
        for p in m.parameters():
            if p.grad is not None:
                p.grad.fill_(1.0)                                                # .grad is a view of the arena
        eng._owned = eng.g32.clone()
    g = torch.randn(eng.total, generator=torch.Generator(device="cpu").manual_seed(seed)) * scale
    eng.g32.copy_(g.to(DEV) * eng._owned)


def bytes_of(t):
    return t.detach().contiguous().view(torch.uint8)


def optimizer_state(opt, shadow=True):
    """Clones of p, m, v (where kept) and, on request, the bf16 shadow - which is no state: a load leaves it to the next refresh."""
    return [t.clone() for t in (opt.eng.q32, opt.m, opt.v, opt.eng.q_lp if shadow else None) if t is not None]


def rel(a, b):
    return float((a.double() - b.double()).norm() / a.double().norm())


# ------------------------------------------------------------------------------------------ parity with torch's optimizers
def torch_optimizer(rule, named, dtype):
    """torch.optim.Adam(groups, lr) / torch.optim.SGD(groups, lr, momentum=0.9) over copies of the parameters in `dtype`, in the
    reference's four groups."""
    copies = {n: p.detach().cpu().to(dtype).clone().requires_grad_(True) for n, p in named}
    def group(decay, head):
        return [copies[n] for n, _ in named if (not any(nd in n for nd in no_decay)) == decay and any(bb in n for bb in head_names) == head]
    groups = [{"params": group(True, False), "weight_decay": WD, "lr": LR}, {"params": group(False, False), "weight_decay": 0.0, "lr": LR},
              {"params": group(True, True), "weight_decay": WD, "lr": LR * LR_MULT}, {"params": group(False, True), "weight_decay": 0.0, "lr": LR * LR_MULT}]
    assert all(len(g["params"]) > 0 for g in groups), [len(g["params"]) for g in groups]     # moco owns a head group: all four are in use
    opt = torch.optim.Adam(groups, lr=LR) if rule == "adam" else torch.optim.SGD(groups, lr=LR, momentum=0.9)
    return copies, opt


@pytest.mark.parametrize("rule", RULES)
def test_three_steps_match_torchs_optimizer(rule):
    m, opt, sched = build(config(optim_type=rule))
    assert type(opt) is vilt_utils.OPTIMIZERS[rule] and opt.rule == rule and not opt.guarded
    assert opt.param_groups[0]["lr"] == LR and (opt.v is None) == (rule == "sgd")     # no warm-up, and the schedule is not stepped below
    eng = m.engine
    before = eng.q32.clone()
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert any("moco_head" in n for n, _ in named) and not any(n.startswith("k_") for n, _ in named)
    c64, o64 = torch_optimizer(rule, named, torch.float64)
    c32, o32 = torch_optimizer(rule, named, torch.float32)
    for step in range(3):
        seeded_grad(m, 40 + step)
        for n, p in named:
            g = p.grad.detach().cpu()                                            # the parameter's view of the gradient arena
            c64[n].grad, c32[n].grad = g.double(), g.clone()
        o64.step()
        o32.step()
        opt.step()
    assert eng.fold_stale["q"] and eng.lpT_stale
    assert opt.t == 3 and opt.counters() == (3, 0)
    worst = ("", 0.0)
    for n, p in named:
        ref = c64[n].detach()
        e32 = float((c32[n].detach().double() - ref).abs().max())
        allowed = FACTOR * max(e32, 2.0 ** -23 * float(ref.abs().max()))
        err = float((p.detach().cpu().double() - ref).abs().max())
        worst = max(worst, (n, err / allowed), key=lambda x: x[1])
        assert err <= allowed, (rule, n, err, allowed, e32)
    print(f"{rule}: largest |got - fp64| / allowed over {len(named)} parameters: {worst[1]:.4f} ({worst[0]})")
    assert not torch.equal(eng.q32, before)
    assert torch.equal(eng.q_lp.view(torch.int16), eng.q32.to(torch.bfloat16).view(torch.int16))     # the bf16 shadow is bf16 of the new weights


# ------------------------------------------------------------------------------------------ the frozen row of an IRTR model
@pytest.mark.parametrize("rule", RULES)
def test_the_frozen_itm_row_keeps_its_bits(rule):
    T.seed_everything(0)
    m = ViLTransformerSS(task_finetune_irtr_coco(num_layers=2, vocab_size=2048, max_steps=10, warmup_steps=0, optim_type=rule, learning_rate=LR,
                                                 weight_decay=WD), device=DEV, compute_dtype="f32")
    opt = m.configure_optimizers()[0][0]
    assert m.engine.irtr and opt.rule == rule and 0.0 in opt.seg_mult.tolist()
    w = dict(m.named_parameters())["itm_score.fc.weight"]
    before = w.detach().clone()
    eng = m.engine
    for step in range(2):
        seeded_grad(m, 50 + step)
        eng.g32[eng.layout.itm_w:eng.layout.itm_w + w.shape[1]] = 1e-3          # not zero on row 0 either: the multiplier alone holds it
        opt.step()
    assert torch.equal(bytes_of(w[0]), bytes_of(before[0]))
    assert not torch.equal(w[1], before[1]) and torch.isfinite(w).all()


# ------------------------------------------------------------------------------------------ state_dict / resume
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("rule", RULES)
def test_round_trip_then_one_more_step_is_bit_equal(rule, guarded, tmp_path):
    cfg = config(optim_type=rule, skip_nonfinite_steps=guarded, gradient_clip_val=5.0 if guarded else 0.0)
    m, opt, sched = build(cfg, seed=0)
    for step in range(3):
        seeded_grad(m, 60 + step)
        opt.step()
        sched.step()
    path = str(tmp_path / f"{rule}.ckpt")
    T.save_checkpoint(path, m, opt, sched, global_step=3, epoch=0, batches_in_epoch=3)
    sd = torch.load(path, map_location="cpu", weights_only=True)["optimizer_states"][0]
    assert sd["rule"] == rule and sd["t"] == 3 and ("v" in sd["state"]) == (rule == "adam")
    m2, opt2, sched2 = build(cfg, seed=77)
    assert not torch.equal(m2.engine.q32, m.engine.q32)
    T.load_checkpoint(path, m2, opt2, sched2)
    assert opt2.t == opt.t == 3 and opt2.counters() == opt.counters() == (3, 0)
    assert opt2.betas == opt.betas and opt2.eps == opt.eps and opt2.param_groups == opt.param_groups
    for a, b in zip(optimizer_state(opt2, shadow=False), optimizer_state(opt, shadow=False)):
        assert torch.equal(bytes_of(a), bytes_of(b))
    for mod, o in ((m, opt), (m2, opt2)):
        seeded_grad(mod, 63)
        o.step()
    for a, b in zip(optimizer_state(opt2), optimizer_state(opt)):
        assert torch.equal(bytes_of(a), bytes_of(b))
    assert opt2.counters() == opt.counters() == (4, 0)


def test_another_rules_state_is_refused_and_an_unnamed_state_is_adamws():
    m, adam, _ = build(config(optim_type="adam"))
    args = (m, LR, WD, LR_MULT)
    sgd, adamw, adam2 = vilt_utils.FusedSGD(*args), vilt_utils.FusedAdamW(*args), vilt_utils.FusedAdam(*args)
    seeded_grad(m, 70)
    adam.step()
    adamw.step()
    with pytest.raises(ValueError) as err:
        sgd.load_state_dict(adam.state_dict())
    assert "'adam'" in str(err.value) and "'sgd'" in str(err.value)
    with pytest.raises(ValueError) as err:
        adam2.load_state_dict(adamw.state_dict())
    assert "'adamw'" in str(err.value) and "'adam'" in str(err.value)
    with pytest.raises(ValueError):
        adamw.load_state_dict(sgd.state_dict())
    assert sgd.t == 0 and adam2.t == 0 and not bool(adam2.m.any()) and not bool(sgd.m.any())          # nothing was written by a refused load
    old = adamw.state_dict()
    del old["rule"]                                                              # a file written before the rule was recorded
    fresh = vilt_utils.FusedAdamW(*args)
    fresh.load_state_dict(old)
    assert fresh.t == 1 and torch.equal(fresh.m, adamw.m) and torch.equal(fresh.v, adamw.v) and float(fresh.v.abs().max()) > 0
    adam2.load_state_dict(adam.state_dict())                                     # (and the same rule loads)
    assert adam2.t == 1 and torch.equal(adam2.v, adam.v)


# ------------------------------------------------------------------------------------------ the guard
@pytest.mark.parametrize("rule", RULES)
def test_a_nan_in_the_gradient_drops_the_step(rule):
    m, opt, sched = build(config(optim_type=rule, skip_nonfinite_steps=True))
    assert opt.guarded
    seeded_grad(m, 80)
    opt.step()
    assert opt.counters() == (1, 0) and opt.grad_norm() > 0 and float(opt.m.abs().max()) > 0
    seeded_grad(m, 81)
    m.engine.g32[12345] = float("nan")
    keep = optimizer_state(opt)
    opt.step()
    for a, b in zip(optimizer_state(opt), keep):
        assert torch.equal(bytes_of(a), bytes_of(b))
    assert opt.counters() == (1, 1) and opt.t == 2
    c = opt.read_ctl()
    assert c.skip == 1 and c.nonfinite == 1
    seeded_grad(m, 82)
    opt.step()                                                                   # the next clean step moves the weights
    assert opt.counters() == (2, 1) and not torch.equal(m.engine.q32, keep[0]) and torch.isfinite(m.engine.q32).all()


# ------------------------------------------------------------------------------------------ trainer
def test_trainer_runs_checkpoints_and_resumes_with_sgd(tmp_path):
    """6 batches, grad_steps = 2: three optimizer steps.  Runs A and A' (uninterrupted, twice) and B (a checkpoint after 4 batches, a
    fresh trainer and model resume from it).  The MoCo step is not bit-reproducible run to run, so B is held to the rule of
    tests/test_resume_gpu.py: its relative distance from A is at most max(1e-5, 10 * distance(A, A')) - for the parameter arena and for
    the momentum arena, which a resume that lost the optimizer state would change by its own size."""
    train = [O.synthetic_batch(OCFG, 4, 200 + i) for i in range(6)]
    val = [O.synthetic_batch(OCFG, 4, 300)]
    over = dict(optim_type="sgd", batch_size=8, max_steps=None, max_epoch=1, learning_rate=1e-3, skip_nonfinite_steps=True)

    def run(tag, seed, **kw):
        cfg = config(**over, **kw)
        T.seed_everything(seed)
        m = ViLTransformerSS(cfg, device=DEV, compute_dtype="bf16")
        validation_step = m.validation_step

        def logged(batch, i):
            out = validation_step(batch, i)
            m.log(T.MONITOR, 0.1)
            return out

        m.validation_step = logged
        tr = T.Trainer(cfg, ckpt_dir=str(tmp_path / tag))
        tr.fit(m, train, val)
        assert type(tr.optimizer) is vilt_utils.FusedSGD and tr.optimizer.v is None
        assert tr.grad_steps == 2 and tr.optimizer.grad_scale == 0.5
        assert tr.global_step == 3 and tr.optimizer.t == 3 and tr.optimizer.counters() == (3, 0) and tr.scheduler.n == 3
        return m.engine.q32.clone(), tr.optimizer.m.clone(), tr.optimizer.param_groups[0]["lr"]

    a, a2 = run("a", 0, val_check_interval=4), run("a2", 0, val_check_interval=4)
    mid = str(tmp_path / "a" / T.BEST)                                           # written by the validation after batch 4: optimizer step 2
    ck = torch.load(mid, map_location="cpu", weights_only=True)
    assert (ck["global_step"], ck["epoch"], ck["batches_in_epoch"]) == (2, 0, 4)
    assert ck["optimizer_states"][0]["rule"] == "sgd" and "v" not in ck["optimizer_states"][0]["state"]
    b = run("b", 9, val_check_interval=4, resume_from=mid)
    assert a[2] == a2[2] == b[2]
    for what, i in (("parameters", 0), ("momentum", 1)):
        noise, dist = rel(a[i], a2[i]), rel(a[i], b[i])
        print(f"sgd resume, {what}: |A - A'| / |A| = {noise:.3e}, |A - B| / |A| = {dist:.3e}")
        assert dist <= max(1e-5, 10 * noise), (what, dist, noise)
    assert float(a[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------ the default is untouched
def test_default_config_still_launches_rmcl_adamw_f32(monkeypatch):
    m, opt, sched = build(config())
    assert m.hparams.config["optim_type"] == "adamw"
    assert type(opt) is vilt_utils.FusedAdamW and opt.rule == "adamw" and opt.betas == (0.9, 0.98) and opt.eps == 1e-8
    assert not opt.guarded and not hasattr(opt, "ctl")
    calls = []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(vilt_utils_lib, name)

    vilt_utils_lib = vilt_utils.lib
    monkeypatch.setattr(vilt_utils, "lib", Recorder())
    seeded_grad(m, 90)
    before = m.engine.q32.clone()
    opt.step()
    assert calls == ["rmcl_adamw_f32"]
    assert opt.counters() == (1, 0) and not torch.equal(m.engine.q32, before)
    with pytest.raises(RuntimeError):
        opt.grad_norm()
