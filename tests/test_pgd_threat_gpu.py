"""-m gpu: the PGD threat models end to end on 2-layer models built from the existing fixtures: the attackers under non-default config keys
(L2 ball, sign step, random start, pixel box) against a torch-autograd loop on the functions of oracle/rmcl_oracle.py, the lane split and
ragged batches under a threat model, ``RobustEval.attack`` / ``curve`` on the toy VQA and NLVR2 fixtures, state restoration and the
config keys.

Oracle parity uses the fp32 engine's ratio of tests/test_vqa_gpu.py (TOL["f32"]: delta 5e-5 at eps = 0.005, loss 1e-3): atol =
1e-2 eps on delta (8-pixel sub-grid), 1e-3 relative on the attacked view's loss.  Under the sign rule an element whose oracle gradient is
below the fp32 engine's tolerance on the data gradient in any step may take the other sign.  That tolerance is 1e-3 of the sample's largest
|g|: the pinned loop steps by adv_lr_img g / max|g| with adv_lr_img = 0.05, and its delta is held to TOL["f32"]["delta"] = 5e-5.
such elements are excluded, and their share - a property of the oracle alone - must stay under 1 %.  Measured values go to the file named
by RMCL_PGD_THREAT_PARITY_OUT when set (profiles/pgd_threat_parity.json is such a dump)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd import RobustEval  # noqa: E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd.attack.pgd_attack_vilt import PGDAttack_moco, PGDAttack_vqa, ThreatModel  # noqa: E402
from rmcl_amd.vilt.config import task_moco, task_finetune_vqa_randaug_attacked  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, vilt_utils  # noqa: E402
from tests import nlvr2_oracle as N  # noqa: E402
from tests import pgd_ball_ref as R  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402
from tests.test_nlvr2_gpu import make_module as make_nlvr2_module  # noqa: E402
from tests.test_path_gpu import build_module, dev_batch  # noqa: E402
from tests.test_vqa_gpu import make_vqa_module  # noqa: E402

DEV = "cuda:0"
PARITY = {}
BOX = (-1.0, 1.0)


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_PGD_THREAT_PARITY_OUT")
    if out and PARITY:
        with open(out, "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------ oracle parity (MoCo, fp32 engine)
def oracle_loop(p, cfg, batch, k, queue, K, lr, eps, norm, rule, box, delta0):
    """K steps of the configured threat model with torch autograd on the oracle's encoder and InfoNCE (CE / K, as the attackers' loop).
    Returns (delta_K, mean CE of the attacked view img + delta_K, per-step gradients)."""
    img0 = batch["image"][0]
    delta, grads = delta0.clone(), []
    for _ in range(K):
        d = delta.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            q, _ = O.encode_q(p, cfg, batch["text_ids"], batch["text_masks"], img0 + d)
            loss = O.infonce_loss(O.infonce_logits(q, k, queue, cfg["temperature"])) / float(K)
            (g,) = torch.autograd.grad(loss, d)
        grads.append(g)
        if norm == "l2":
            dirn = g / g.flatten(1).norm(dim=1).clamp_min(1e-12).view(-1, 1, 1, 1)
        elif rule == "sign":
            dirn = g.sign()
        else:
            dirn = g / g.abs().flatten(1).max(dim=1).values.clamp_min(1e-8).view(-1, 1, 1, 1)
        t = delta + lr * dirn
        if norm == "l2":
            t = t * (eps / t.flatten(1).norm(dim=1).clamp_min(1e-30)).clamp(max=1.0).view(-1, 1, 1, 1)
        else:
            t = t.clamp(-eps, eps)
        delta = ((img0 + t).clamp(*box) - img0) if box is not None else t
        delta = delta.detach()
    with torch.no_grad():
        q, _ = O.encode_q(p, cfg, batch["text_ids"], batch["text_masks"], img0 + delta)
        ce = O.infonce_loss(O.infonce_logits(q, k, queue, cfg["temperature"]))
    return delta, float(ce), grads


def moco_case():
    ocfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=2, adv_steps_img=2)
    m, p = build_module(ocfg, 21, "f32")
    batch = O.synthetic_batch(ocfg, 2, 22)
    batch["image"] = [batch["image"][0].clamp(-1.0, 1.0)]                       # pixels of the pixelbert range: base lies in the box
    g = torch.Generator().manual_seed(23)
    k = torch.nn.functional.normalize(torch.randn(2, 128, generator=g), dim=1)
    return ocfg, m, p, batch, k


def engine_attack(m, batch, k, **keys):
    att = PGDAttack_moco(dict(m.config, **keys))
    b = dev_batch(batch)
    img0 = b["image"][0].clone()
    eng = m.engine
    seed = att.threat.step_seed(eng)
    delta = att.pgd_attack(m, b, k_modality=k.to(DEV))
    pb = eng.bufs(2)
    # the loss of the attacked view the loop left in patchesT_full: one inference forward + InfoNCE rows
    from rmcl_amd.task_loss import InfoNceLoss
    rows = InfoNceLoss(m, metrics=False).forward(pb, pb.patchesT_full, L.MODE_INFER, want_grad=False, scale=0.0, wgrad=False)
    return delta, float(rows.mean()), b["image"][0], img0, seed, pb


def test_l2_box_attack_matches_the_autograd_oracle():
    ocfg, m, p, batch, k = moco_case()
    eps, lr, K = 1.0, 0.7, 2                                                   # two steps of 0.7 eps from 0: the second leaves the ball
    delta, ce, left, img0, _, _ = engine_attack(m, batch, k, adv_norm_img="l2", adv_pixel_box_img=BOX, adv_steps_img=K, adv_lr_img=lr,
                                                adv_max_norm_img=eps)
    torch.set_num_threads(16)
    want, want_ce, _ = oracle_loop(p, ocfg, batch, k, O.init_queue(ocfg, 0), K, lr, eps, "l2", None, BOX, torch.zeros_like(batch["image"][0]))
    dev = float((delta.cpu() - want)[:, :, ::8, ::8].abs().max())
    PARITY["l2_box"] = {"delta_max_dev_sub": dev, "delta_atol": 1e-2 * eps, "loss": ce, "oracle_loss": want_ce, "loss_rel_dev": abs(ce - want_ce) / want_ce}
    print(PARITY["l2_box"])
    assert dev <= 1e-2 * eps and abs(ce - want_ce) <= 1e-3 * want_ce
    nrm = delta.double().flatten(1).norm(dim=1)
    assert bool((nrm <= eps * (1 + 2.0 ** -22)).all())
    unboxed, _, _ = oracle_loop(p, ocfg, batch, k, O.init_queue(ocfg, 0), K, lr, eps, "l2", None, None, torch.zeros_like(batch["image"][0]))
    un = unboxed.double().flatten(1).norm(dim=1)
    assert bool(((un - eps).abs() <= 1e-5 * eps).all())                        # the projection did bind: without the box delta_K lies ON the sphere
    assert torch.equal(left, img0 + delta) and float(left.max()) <= 1.0 and float(left.min()) >= -1.0      # img + delta_K is left behind


def test_random_start_sign_attack_matches_the_autograd_oracle():
    ocfg, m, p, batch, k = moco_case()
    eps, lr, K, seed = 0.005, 0.002, 2, 5
    delta, ce, left, img0, used_seed, pb = engine_attack(m, batch, k, adv_step_rule_img="sign", adv_random_start_img=True, adv_seed_img=seed,
                                                         adv_steps_img=K, adv_lr_img=lr, adv_max_norm_img=eps)
    # the start, from the numpy hash, through the engine's own patch -> image layout
    per = pb.d.P * pb.d.patch_k
    d0p = torch.from_numpy(R.random_start_linf_f32(2, per, 0, used_seed, eps)[0]).to(DEV).view_as(pb.delta)
    delta0 = m.engine.patches_to_image(d0p, pb).cpu()
    assert float(delta0.abs().max()) <= eps and float(delta0.abs().mean()) > 0.4 * eps
    torch.set_num_threads(16)
    want, want_ce, grads = oracle_loop(p, ocfg, batch, k, O.init_queue(ocfg, 0), K, lr, eps, "linf", "sign", None, delta0)
    unsure = torch.zeros_like(want, dtype=torch.bool)
    for g in grads:
        unsure |= g.abs() < 1e-3 * g.abs().flatten(1).max(dim=1).values.view(-1, 1, 1, 1)
    share = float(unsure.float().mean())
    ok = ~unsure[:, :, ::8, ::8]
    dev = float(((delta.cpu() - want)[:, :, ::8, ::8].abs() * ok).max())
    PARITY["random_start_sign"] = {"delta_max_dev_sub": dev, "delta_atol": 1e-2 * eps, "excluded_share": share, "loss": ce, "oracle_loss": want_ce,
                                   "loss_rel_dev": abs(ce - want_ce) / want_ce}
    print(PARITY["random_start_sign"])
    assert share < 0.01
    assert dev <= 1e-2 * eps and abs(ce - want_ce) <= 1e-3 * want_ce
    assert float(delta.abs().max()) <= R.f32(eps) and torch.equal(left, img0 + delta)


def test_moco_step_under_random_start_takes_its_clean_query_from_a_forward_of_its_own():
    """compute_moco_contrastive fuses the clean query forward into PGD step 0 (dropout off, image view only).  Under a random start step 0
    no longer sees the clean image: q_original must still be the clean query - the oracle's, and the default-key step's."""
    ocfg, m, p, batch, _ = moco_case()
    db = dev_batch(batch)
    q = {}
    for name, keys in (("default", {}), ("random_start", dict(adv_random_start_img=True, adv_step_rule_img="sign", adv_pixel_box_img=BOX))):
        m.pgd_attacker = PGDAttack_moco(dict(m.config, **keys))
        m.queue_ptr = 0
        m.proj_queue.copy_(O.init_queue(ocfg, 0).to(DEV))
        vilt_utils.set_task(m)
        ret = m(db)
        torch.cuda.synchronize()
        q[name] = ret["q_original"].detach().clone()
        assert bool(torch.isfinite(ret["moco_loss"]).all()) and float(m.engine.bufs(2).delta.abs().max()) > 0
    with torch.no_grad():
        want, _ = O.encode_q(p, ocfg, batch["text_ids"], batch["text_masks"], batch["image"][0])
    assert float((q["random_start"].cpu() - want).abs().max()) <= 1e-4            # (the fp32 engine's tolerance on cls features: tests/test_path_gpu.py)
    assert float((q["random_start"] - q["default"]).abs().max()) <= 1e-5          # an inference forward against step 0's MODE_DATA forward
    PARITY["moco_clean_query"] = {"vs_oracle": float((q["random_start"].cpu() - want).abs().max()), "vs_default_step": float((q["random_start"] - q["default"]).abs().max())}


def test_bf16_engine_keeps_ball_box_and_pads():
    ocfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=4, adv_steps_img=2)
    m, _ = build_module(ocfg, 21, "bf16")
    sizes = [(384, 352), (320, 384), (384, 384), (224, 288)]
    batch = O.synthetic_batch(ocfg, 4, 22, sizes=sizes)
    batch["image"] = [batch["image"][0].clamp(-1.0, 1.0)]
    k = torch.nn.functional.normalize(torch.randn(4, 128, generator=torch.Generator().manual_seed(3)), dim=1).to(DEV)
    for keys, eps in ((dict(adv_norm_img="l2", adv_random_start_img=True), 1.0), (dict(adv_step_rule_img="sign", adv_random_start_img=True), 0.005)):
        att = PGDAttack_moco(dict(m.config, adv_pixel_box_img=BOX, adv_steps_img=3, adv_lr_img=eps / 2, adv_max_norm_img=eps, **keys))
        b = dev_batch(batch)
        pb = m.engine.bind_batch(b["text_ids"], b["text_masks"], b["image"][0], tag="moco")
        delta = att.attack_patches(m, pb, k)
        assert delta.data_ptr() == pb.delta.data_ptr() and float(delta.abs().max()) > 0 and bool(torch.isfinite(delta).all())
        if "adv_norm_img" in keys:
            assert bool((pb.delta.double().view(4, -1).norm(dim=1) <= eps * (1 + 2.0 ** -22)).all())
        else:
            assert float(pb.delta.abs().max()) <= R.f32(eps) + 2.0 ** -23
        # pads: delta 0 and the operand the clean cast, through K = 3 steps (ragged batch: counts * patch_k leading elements are valid)
        valid = m.engine.pgd_valid(pb)
        assert valid is not None and int(valid.min()) < pb.d.P * pb.d.patch_k
        pad = torch.arange(pb.d.P * pb.d.patch_k, device=DEV)[None, :] >= valid[:, None].to(torch.int64)
        assert bool(pad.any()) and float(pb.delta.view(4, -1)[pad].abs().max()) == 0.0
        clean = pb.patches32.to(torch.bfloat16).view(4, -1)
        full = pb.patchesT_full.view(4, -1)
        assert torch.equal(full[pad].view(torch.int16), clean[pad].view(torch.int16))
        x = full[~pad].float()
        assert float(x.max()) <= 1.0 and float(x.min()) >= -1.0


def test_lane_split_equals_the_one_chain_run_under_random_start(monkeypatch):
    ocfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=4, adv_steps_img=2)
    m, _ = build_module(ocfg, 5, "bf16")
    m.engine.cfg["dense_images"] = True
    batch = O.synthetic_batch(ocfg, 4, 9, ragged_text=True)
    batch["image"] = [batch["image"][0].clamp(-1.0, 1.0)]
    k = torch.nn.functional.normalize(torch.randn(4, 128, generator=torch.Generator().manual_seed(3)), dim=1).to(DEV)
    out = {}
    for norm, eps in (("linf", 0.005), ("l2", 1.0)):
        for lanes in ("0", "1"):
            monkeypatch.setenv("RMCL_LANES", lanes)
            m.engine.pass_counter = 100                                           # the same seed for both runs
            att = PGDAttack_moco(dict(m.config, adv_norm_img=norm, adv_step_rule_img="sign", adv_random_start_img=True, adv_pixel_box_img=BOX,
                                      adv_steps_img=2, adv_lr_img=eps / 2, adv_max_norm_img=eps, adv_seed_img=7))
            att.pgd_attack(m, dev_batch(batch), k_modality=k)
            torch.cuda.synchronize()
            pb = m.engine.bufs(4)
            assert (getattr(pb, "_lanes", None) is not None) or lanes == "0"
            out[lanes] = (pb.delta.clone(), pb.patchesT_full.clone())
        assert getattr(m.engine.bufs(4), "_lanes", None) is not None, "the lanes did not run"
        assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1].view(torch.int16), out["1"][1].view(torch.int16)), norm
        assert float(out["0"][0].abs().max()) > 0


# ------------------------------------------------------------------------------------------ RobustEval
def vqa_model(dtype="f32", **over):
    g, cfg, p, batch, targets, _ = V.load_case("vqa_L2_B4_ragged")
    return make_vqa_module(cfg, p, dtype, **over), batch


def check_ball_and_box(res, imgs, eps, norm):
    deltas = res["delta"] if isinstance(res["delta"], tuple) else (res["delta"],)
    for d, img in zip(deltas, imgs):
        if norm == "l2":
            assert bool((d.double().flatten(1).norm(dim=1) <= eps * (1 + 2.0 ** -22)).all())
        else:
            assert float(d.abs().max()) <= R.f32(eps) + 2.0 ** -23
        x = img + d
        assert float(x.max()) <= 1.0 + 2.0 ** -23 and float(x.min()) >= -1.0 - 2.0 ** -23


@pytest.mark.parametrize("norm,eps", [("linf", 0.01), ("l2", 2.0)])
def test_robust_eval_attack_vqa(norm, eps):
    m, batch = vqa_model()
    batch["image"] = [batch["image"][0].clamp(-1.0, 1.0)]
    db = dev_batch(batch)
    B = db["text_ids"].shape[0]
    re = RobustEval(m)
    r1 = re.attack(db, eps, norm=norm, steps=3, restarts=1, seed=4)
    r3 = re.attack(db, eps, norm=norm, steps=3, restarts=3, seed=4)
    # the clean numbers are compute_vqa's for the same batch
    m.eval()
    vilt_utils.set_task(m)
    with torch.no_grad():
        out = m(db)
    vb = m.engine.vqa_bufs(B, "vqa")
    assert torch.equal(r1["clean_pred"], out["vqa_preds"].to(torch.int32)) and torch.equal(r1["clean_pred"], r3["clean_pred"])
    assert torch.equal(r1["clean_loss"], vb.rows[:, 0]) and torch.equal(r1["clean_score"], vb.rows[:, 1])
    assert abs(float(r1["clean_score"].mean()) - float(m.logged["vqa/val/score"])) < 1e-6
    check_ball_and_box(r1, [db["image"][0]], eps, norm)
    check_ball_and_box(r3, [db["image"][0]], eps, norm)
    assert float(r1["delta"].abs().max()) > 0 and bool((r1["adv_loss"] > r1["clean_loss"]).any())
    # restart 0 of the 3-restart run is the 1-restart run; the worst case over restarts never has a smaller loss
    assert bool((r3["adv_loss"] >= r1["adv_loss"]).all())
    assert bool(((r3["best_restart"] >= 0) & (r3["best_restart"] <= 2)).all()) and bool((r1["best_restart"] == 0).all())
    same = r3["best_restart"] == 0                                          # every sample is checked: it kept restart 0's bits, or left for a larger loss
    assert torch.equal(r3["delta"][same], r1["delta"][same]) and torch.equal(r3["adv_loss"][same], r1["adv_loss"][same])
    assert bool(same.any()) and bool((r3["adv_loss"][~same] > r1["adv_loss"][~same]).all())
    again = re.attack(db, eps, norm=norm, steps=3, restarts=1, seed=4)
    assert torch.equal(again["delta"], r1["delta"]) and torch.equal(again["adv_loss"], r1["adv_loss"])
    other = re.attack(db, eps, norm=norm, steps=3, restarts=1, seed=5)
    assert not torch.equal(other["delta"], r1["delta"])
    PARITY[f"robust_vqa/{norm}"] = {"clean_loss": r1["clean_loss"].tolist(), "adv_loss_r1": r1["adv_loss"].tolist(), "adv_loss_r3": r3["adv_loss"].tolist(),
                                    "best_restart": r3["best_restart"].tolist()}


@pytest.mark.parametrize("pair", [True, False])
def test_robust_eval_attack_nlvr2(pair):
    cfg, p, batch, _ = N.case_inputs("nlvr2_att_K2_L2_B4_idx10")
    m = make_nlvr2_module(cfg, p, "f32", attack_idx=[True, False], nlvr2_pair_pass=pair)
    for key in ("image_0", "image_1"):
        batch[key] = [batch[key][0].clamp(-1.0, 1.0)]
    db = dev_batch(batch)
    B = db["text_ids"].shape[0]
    re = RobustEval(m)
    eps = 0.01
    r1 = re.attack(db, eps, steps=3, restarts=1, seed=2)
    r3 = re.attack(db, eps, steps=3, restarts=3, seed=2)
    m.eval()
    vilt_utils.set_task(m)
    with torch.no_grad():
        m(db)
    nb = m.engine.nlvr2_bufs(B, "nlvr2")
    assert torch.equal(r1["clean_pred"], nb.argmax) and torch.equal(r1["clean_loss"], nb.rows)
    assert torch.equal(r1["clean_score"], (nb.argmax == nb.labels).float())
    check_ball_and_box(r3, [db["image_0"][0], db["image_1"][0]], eps, "linf")
    d0, d1 = r3["delta"]
    assert float(d0.abs().max()) > 0 and float(d1.abs().max()) == 0.0                     # attack_idx = [True, False]: image_1 is never moved
    assert bool((r3["adv_loss"] >= r1["adv_loss"]).all()) and bool(((r3["best_restart"] >= 0) & (r3["best_restart"] <= 2)).all())
    same = r3["best_restart"] == 0
    assert torch.equal(r3["delta"][0][same], r1["delta"][0][same]) and torch.equal(r3["adv_loss"][same], r1["adv_loss"][same])
    assert bool((r3["adv_loss"][~same] > r1["adv_loss"][~same]).all())
    # both images attacked: every pair's two deltas come from the same restart (each restart's deltas are told apart by their bits)
    m2 = make_nlvr2_module(cfg, p, "f32", attack_idx=[True, True], nlvr2_pair_pass=pair)
    re2 = RobustEval(m2)
    full = re2.attack(db, eps, steps=2, restarts=3, seed=2)
    singles = [re2.attack(db, eps, steps=2, restarts=1, seed=2)]
    assert bool((full["delta"][1].abs().flatten(1).max(dim=1).values > 0).all())
    r0 = full["best_restart"] == 0
    for k in range(2):                                                                    # image k of pair b differs from restart 0's iff b left restart 0
        assert torch.equal(full["delta"][k][r0], singles[0]["delta"][k][r0])
        moved = (full["delta"][k] != singles[0]["delta"][k]).flatten(1).any(dim=1)
        assert torch.equal(moved, ~r0), k


def test_curve_and_eps_zero():
    m, batch = vqa_model()
    batch["image"] = [batch["image"][0].clamp(-1.0, 1.0)]
    db = dev_batch(batch)
    half = lambda s: {k: ([v[0][s]] if k == "image" else v[s]) for k, v in db.items()}
    batches = [half(slice(0, 2)), half(slice(2, 4))]
    re = RobustEval(m)
    rows = re.curve(batches, eps=[0.0, 0.02], steps=2, restarts=2, seed=1)
    assert [r["eps"] for r in rows] == [0.0, 0.02] and all(r["n"] == 4 for r in rows)
    assert rows[0]["clean_score"] == rows[1]["clean_score"] and rows[0]["clean_loss"] == rows[1]["clean_loss"]
    assert rows[0]["robust_score"] == rows[0]["clean_score"] and rows[0]["flip_rate"] == 0.0 and rows[0]["adv_loss"] == rows[0]["clean_loss"]
    assert rows[1]["adv_loss"] > rows[1]["clean_loss"] and 0.0 <= rows[1]["flip_rate"] <= 1.0
    # the same numbers as attack() batch by batch
    parts = [re.attack(b, 0.02, steps=2, restarts=2, seed=1) for b in batches]
    adv = torch.cat([p["adv_loss"] for p in parts]).double().mean()
    assert abs(float(adv) - rows[1]["adv_loss"]) <= 1e-6 * float(adv)
    z = re.attack(db, 0.0)
    assert float(z["delta"].abs().max()) == 0.0 and torch.equal(z["adv_loss"], z["clean_loss"]) and torch.equal(z["adv_pred"], z["clean_pred"])
    PARITY["curve_vqa"] = rows


def test_an_evaluation_leaves_no_engine_state_behind():
    """Identical models under dropout: the training step after RobustEval.attack has the loss bits of the same step without it."""
    g, cfg, p, batch, _, _ = V.load_case("vqa_L2_B4_ragged")
    losses = []
    for evaluate_first in (False, True):
        torch.manual_seed(3)
        m = make_vqa_module(cfg, p, "bf16", drop_rate=0.1)
        m.train()
        db = dev_batch(batch)
        if evaluate_first:
            RobustEval(m).attack(db, 0.01, steps=2, restarts=2)
            assert m.training and all(mod.training for mod in m.modules())
        m.zero_grad()
        loss = m.training_step(db, 0)
        loss.backward()
        torch.cuda.synchronize()
        losses.append(loss.detach().clone())
    assert torch.isfinite(losses[0]) and torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32))


def test_a_model_without_a_task_head_is_refused():
    m = ViLTransformerSS(task_moco(num_layers=1, num_negative=1024, per_gpu_batchsize=2, image_view=True), device=DEV, compute_dtype="f32")
    with pytest.raises(ValueError, match="neither"):
        RobustEval(m)


# ------------------------------------------------------------------------------------------ config
def test_config_keys():
    base = task_finetune_vqa_randaug_attacked(image_view=True, num_layers=1)
    assert ThreatModel.from_config(base).is_default and base["adv_norm_img"] == "linf" and base["adv_pixel_box_img"] is None
    for bad in (dict(adv_norm_img="l1"), dict(adv_step_rule_img="fgsm"), dict(adv_random_start_img="yes"), dict(adv_pixel_box_img=(1.0, -1.0)),
                dict(adv_pixel_box_img=0.5), dict(adv_seed_img=1.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            PGDAttack_vqa(dict(base, **bad))
    assert ThreatModel("l2", "sign").direction == L.PGD_DIR_L2                                    # the step rule is ignored for l2


def test_default_keys_write_the_bytes_of_a_config_without_them():
    g, cfg, p, batch, _, _ = V.load_case("vqa_att_K2_L2_B4_ragged")
    deltas = []
    for strip in (False, True):
        m = make_vqa_module(cfg, p, "f32", attacked=True)
        if strip:                                                                                  # a config dict from before the keys existed
            conf = {k: v for k, v in m.config.items() if k not in ("adv_norm_img", "adv_step_rule_img", "adv_random_start_img",
                                                                    "adv_pixel_box_img", "adv_seed_img")}
            m.pgd_attacker = PGDAttack_vqa(conf)
        assert m.pgd_attacker.threat.is_default
        m.zero_grad()
        m.training_step(dev_batch(batch), 0)
        torch.cuda.synchronize()
        deltas.append(m.engine.bufs(cfg["per_gpu_batchsize"], "vqa_att").delta.clone())
    assert float(deltas[0].abs().max()) > 0 and torch.equal(deltas[0].view(torch.int32), deltas[1].view(torch.int32))
