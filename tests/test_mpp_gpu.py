"""-m gpu: masked patch prediction (task_mlm_itm_mpp) at the module level - the whole mpp and mlm + itm + mpp steps against the
reference's own run (tests/golden/mpp_*.npz, mlm_itm_mpp_L2_B4.npz from tools/gen_golden_mpp.py), task composition, the unchanged
models without the head, and the public surface: infer(mask_image=True), the state dict, pixel validation, training, epoch accuracy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd.vilt.config import task_mlm_itm, task_mlm_itm_mpp, task_moco, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from tests import mlm_oracle as ML  # noqa: E402
from tests import mpp_oracle as M  # noqa: E402
from tests.golden_util import digest  # noqa: E402
from tests.test_mlm_gpu import TOL, compare_with_golden as mlm_compare_with_golden  # noqa: E402  (the bounds of the MLM golden tests)
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"


def make_module(ocfg, p, dtype="f32", mlm=False, itm=False, mpp=True, **over):
    kw = dict(num_layers=ocfg["num_layers"], per_gpu_batchsize=ocfg["per_gpu_batchsize"], drop_rate=0.0, max_steps=100, warmup_steps=0,
              loss_names=_loss_names({"mlm": int(mlm), "itm": int(itm), "mpp": int(mpp)}))
    kw.update(over)
    m = ViLTransformerSS(task_mlm_itm_mpp(**kw), device=DEV, compute_dtype=dtype)
    skip = ("k_", "moco_head") + (() if itm else ("itm_score",)) + (() if mlm else ("mlm_score",)) + (() if mpp else ("mpp_score", "transformer.mask_token"))
    sd = {n: t.detach().to(DEV) for n, t in p.items() if not n.startswith(skip)}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    m.train()
    return m


def with_masks(batch, masked, replaced):
    b = dict(batch)
    b["mpp_masked"], b["mpp_replaced"] = masked, replaced
    return b


def _step(m, batch):
    m.zero_grad()
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    return loss


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", M.FIXTURES)
def test_mpp_step_matches_reference_golden(name, dtype):
    g, cfg, p, batch, masked, replaced, with_mlm_itm = M.load_case(name)
    tol = TOL[dtype]
    m = make_module(cfg, p, dtype, mlm=with_mlm_itm, itm=with_mlm_itm)
    if with_mlm_itm:
        m.itm_labels_override = torch.from_numpy(g["itm_labels"])
    db = with_masks(dev_batch(batch), masked, replaced)
    loss = _step(m, db)
    B, n = cfg["per_gpu_batchsize"], int(g["n"])
    eng = m.engine
    mp = eng.mpp_bufs(B, "mpp", g["image_labels"].shape[1] - 1)
    assert mp.count.tolist() == [n, 0]
    out = m(db)
    assert out["mpp_logits"] is None and np.array_equal(out["mpp_labels"].cpu().numpy(), g["image_labels"])     # image_labels: equal
    mpp_loss = float(m.logged["mpp/train/loss"])
    params = dict(m.named_parameters())
    if n == 0:
        assert np.isnan(float(g["mpp_loss"])) and np.isnan(mpp_loss) and np.isnan(float(loss))
        for nm, prm in params.items():                                    # the empty fixture: untouched gradients
            assert torch.count_nonzero(prm.grad) == 0 and bool(torch.isfinite(prm.grad).all()), nm
        return
    bad, obs = [], {}

    def chk(key, err, bound):
        obs[key] = float(err)
        if not err <= bound:
            bad.append((key, float(err), float(bound)))

    chk("loss_rel", abs(float(loss) - float(g["total_loss"])) / float(g["total_loss"]), tol["loss"])
    chk("mpp_loss_rel", abs(mpp_loss - float(g["mpp_loss"])) / float(g["mpp_loss"]), tol["loss"])
    zmax = max(1.0, float(g["zmax"]))
    rl = mp.rowloss[:n].cpu().numpy()
    chk("row_loss_abs_over_max", np.abs(rl - g["row_loss"].sum(1)).max() / max(1.0, np.abs(g["row_loss"].sum(1)).max()), tol["loss"])
    lg = eng.mpp_logits(mp, n).cpu().numpy()
    chk("logits_abs_over_zmax", np.abs(lg - g["row_logits"]).max() / zmax, tol["logits"])
    # argmax / accuracy: integers, exact in f32.  bf16: a pair may differ only where the REFERENCE's top-two gap is below the logits
    # tolerance (the generator asserts the reference has no such pair)
    am = mp.argmax[:n].cpu().numpy()
    differ = am != g["argmax"]
    near = g["gap"] < tol["logits"] * zmax
    assert not near.any()
    assert not (differ & ~near).any(), ("argmax differs on a pair with a clear gap", np.argwhere(differ & ~near))
    assert int(round(float(m.logged["mpp/train/accuracy"]) * 3 * n)) == int(g["correct"])
    assert abs(float(m.logged["mpp/train/accuracy"]) - float(g["log_accuracy"])) < 1e-6
    if with_mlm_itm:
        chk("itm_loss_rel", abs(float(m.logged["itm/train/loss"]) - float(g["itm_loss"])) / float(g["itm_loss"]), tol["loss"])
        chk("mlm_loss_rel", abs(float(m.logged["mlm/train/loss"]) - float(g["mlm_loss"])) / float(g["mlm_loss"]), tol["loss"])
    worst = 0.0
    for nm, d in zip(g["grad_names"], g["grad_digest"]):
        got = digest(params[str(nm)].grad)
        e = abs(got[1] - d[1]) / (d[1] + 1e-30)
        worst = max(worst, e)
        if not abs(got[1] - d[1]) <= tol["grad"] * d[1] + 1e-7:
            bad.append(("grad_digest " + str(nm), float(e), tol["grad"]))
    obs["grad_digest_l2_rel_worst"] = worst
    slices = (("grad_mask_token", params["transformer.mask_token"].grad.flatten()),
              ("grad_decoder_w", params["mpp_score.decoder.weight"].grad[::48, :64]), ("grad_decoder_b", params["mpp_score.decoder.bias"].grad),
              ("grad_dense_w", params["mpp_score.transform.dense.weight"].grad[:8, :64]),
              ("grad_patch_w", params["transformer.patch_embed.proj.weight"].grad.reshape(768, -1)[:8, :64]),
              ("grad_patch_b", params["transformer.patch_embed.proj.bias"].grad))
    for key, got in slices:
        ref = g[key]
        chk(key + "_abs_over_max", np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max(), tol["grad"] * 2.5)
    print(name, dtype, obs)
    assert not bad, bad
    # dense logits under no_grad in eval mode: [B, 1 + P, 3, 256], and they agree with the compacted statistics
    m.eval()
    with torch.no_grad():
        oe = m(db)
    lgd = oe["mpp_logits"]
    P1 = g["image_labels"].shape[1]
    assert tuple(lgd.shape) == (B, P1, 3, 256)
    on = torch.from_numpy((g["image_labels"] != -100).any(-1)).to(DEV)
    rows = lgd[on]                                                           # [n, 3, 256]
    assert torch.equal(rows.argmax(dim=2).to(torch.int32), eng.mpp_bufs(B, "mpp", P1 - 1).argmax[:n])
    ref_loss = torch.nn.functional.cross_entropy(rows.double().reshape(-1, 256), torch.from_numpy(g["labels"]).to(DEV).reshape(-1))
    assert abs(float(oe["mpp_loss"]) - float(ref_loss)) < 1e-5 * float(ref_loss)


def test_mlm_itm_mpp_gradients_are_the_sum_of_the_single_task_gradients():
    """drop_rate = 0, ITM labels and masks fixed: the three deferred backwards accumulate into the one arena (fp32 accumulation order only)"""
    g, cfg, p, batch, masked, replaced, _ = M.load_case("mlm_itm_mpp_L2_B4")
    lab = torch.from_numpy(g["itm_labels"])
    grads = {}
    for key, (wm, wi, wp) in (("all", (True, True, True)), ("mlm", (True, False, False)), ("itm", (False, True, False)), ("mpp", (False, False, True))):
        m = make_module(cfg, p, "f32", mlm=wm, itm=wi, mpp=wp)
        m.itm_labels_override = lab
        _step(m, with_masks(dev_batch(batch), masked, replaced))
        grads[key] = {n_: prm.grad.clone() for n_, prm in m.named_parameters() if prm.grad is not None}
        del m
    for n_, gb in grads["all"].items():
        want = sum(grads[k][n_] for k in ("mlm", "itm", "mpp") if n_ in grads[k])
        err = float((gb - want).abs().max())
        assert err <= 2e-6 * float(want.abs().max()) + 1e-30, (n_, err, float(want.abs().max()))


def test_models_without_mpp_are_unchanged():
    m = ViLTransformerSS(task_mlm_itm(num_layers=2, per_gpu_batchsize=2), device=DEV, compute_dtype="f32")
    eng = m.engine
    assert eng.mpp is None and not eng.mpp_specs
    assert eng.total == int(eng.layout.total) + sum((int(np.prod(s)) + 63) // 64 * 64 for _, _, s in eng.mlm_specs)
    assert not any("mpp" in k or "mask_token" in k for k in m.state_dict())
    k = ViLTransformerSS(task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=2, image_view=True), device=DEV, compute_dtype="f32")
    assert k.engine.mpp is None and k.engine.total == int(k.engine.layout.total) and not any("mask_token" in n for n in k.state_dict())
    # the mlm + itm step still lands on its own reference fixture
    obs, bad, *_ = mlm_compare_with_golden("mlm_itm_L2_B4", "f32")
    assert not bad, bad
    # ... and is the SAME step whether the config comes from task_mlm_itm or from task_mlm_itm_mpp with mpp switched off: equal specs and
    # arena, and after one step from the same seeds equal bits in everything computed without float atomics (the MLM loss and accuracy, the encoder
    # output, the MLM head's per-row outputs and its six gradients, which read the whole forward); the other gradients meet in float
    # atomics (weight-gradient split-K, column sums: their order changes from run to run), so their digests agree to that order only
    g, cfg, p, batch, _ = ML.load_case("mlm_itm_L2_B4")
    got = {}
    for key, task in (("plain", task_mlm_itm), ("mpp_off", task_mlm_itm_mpp)):
        mm = ViLTransformerSS(task(num_layers=2, per_gpu_batchsize=4, drop_rate=0.0, max_steps=100, warmup_steps=0, max_image_len=200,
                                   datasets=["coco"], exp_name="x", loss_names=_loss_names({"mlm": 1, "itm": 1})), device=DEV, compute_dtype="f32")
        mm.load_state_dict({n: t.to(DEV) for n, t in p.items() if not n.startswith(("k_", "moco_head"))}, strict=True)
        mm.train()
        mm.itm_labels_override = torch.from_numpy(g["itm_labels"])
        loss = _step(mm, dev_batch(batch))
        mb = mm.engine.mlm_bufs(4, "mlm")
        got[key] = dict(cfg=mm.hparams.config, specs=list(mm.engine.specs), total=mm.engine.total, loss=loss.detach().clone(),
                        logged={k: float(v) for k, v in mm.logged.items()}, xn=mm.engine.bufs(4, "itm").xn.clone(),
                        rowloss=mb.rowloss[:mb.rows].clone(), argmax=mb.argmax[:mb.rows].clone(),       # (the launch extent: what the kernels write)
                        grads={n: digest(prm.grad) for n, prm in mm.named_parameters() if prm.grad is not None})
        del mm
    a, b = got["plain"], got["mpp_off"]
    assert a["cfg"] == b["cfg"] and a["specs"] == b["specs"] and a["total"] == b["total"]
    for k in a["logged"]:                                                   # (the ITM loss and the WPA distance are summed by float atomics)
        if k.startswith("mlm/"):
            assert a["logged"][k] == b["logged"][k], k
        else:
            assert abs(a["logged"][k] - b["logged"][k]) <= 1e-6 * abs(a["logged"][k]) + 1e-30, k
    assert sorted(a["logged"]) == sorted(b["logged"]) and abs(float(a["loss"]) - float(b["loss"])) <= 1e-6 * float(a["loss"])
    assert torch.equal(a["xn"], b["xn"]) and torch.equal(a["rowloss"], b["rowloss"]) and torch.equal(a["argmax"], b["argmax"])
    assert sorted(a["grads"]) == sorted(b["grads"])
    for n in a["grads"]:
        if n.startswith("mlm_score."):
            assert np.array_equal(a["grads"][n], b["grads"][n]), n
        else:
            assert abs(a["grads"][n][1] - b["grads"][n][1]) <= 1e-6 * a["grads"][n][1] + 1e-30, n
    db = dev_batch(O.synthetic_batch(O.default_config(num_layers=2), 2, 3))
    with pytest.raises(NotImplementedError):
        m.infer(db, mask_image=True)
    with pytest.raises(NotImplementedError):
        m.visual_embed(db["image"][0], mask_it=True)


def test_public_surface_of_an_mpp_model(tmp_path):
    g, cfg, p, batch, masked, replaced, _ = M.load_case("mpp_L2_B4_ragged")
    m = make_module(cfg, p, "f32")
    db = with_masks(dev_batch(batch), masked, replaced)
    with torch.no_grad():
        out = m.infer(db, mask_image=True)
        r = M.infer_masked(p, cfg, batch["text_ids"], batch["text_masks"], batch["image"][0], replaced)
    P1 = g["image_labels"].shape[1]
    assert tuple(out["image_labels"].shape) == (4, P1, 3) and np.array_equal(out["image_labels"].cpu().numpy(), g["image_labels"])
    on = r["image_masks"].bool()
    assert tuple(out["image_feats"].shape) == (4, P1, 768)
    assert float((out["image_feats"].cpu()[on] - r["image_feats"][on]).abs().max()) < 2e-3 * max(1.0, float(r["image_feats"].abs().max()))
    for kw in (dict(mask_text=True), dict(image_embeds=out["image_feats"], image_masks=out["image_masks"])):
        with pytest.raises(NotImplementedError):
            m.infer(db, mask_image=True, **kw)
    with pytest.raises(NotImplementedError):
        m.infer_k(db, mask_image=True)
    # without injected masks the draw comes from torch's CPU generator, in the reference's order
    torch.manual_seed(11)
    with torch.no_grad():
        o2 = m.infer(dev_batch(batch), mask_image=True)
    torch.manual_seed(11)
    mk = torch.bernoulli(torch.full((4, 144), 0.15)).bool()
    assert np.array_equal(o2["image_labels"].cpu().numpy(), M.image_labels(batch["image"][0], cfg, mk).numpy())
    # the state dict carries transformer.mask_token and mpp_score.*, survives a save and loads through load_path
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    for k in M.HEAD:
        assert torch.equal(sd[k], p[k]), k
    path = str(tmp_path / "mpp.ckpt")
    torch.save({"state_dict": sd}, path)
    m2 = ViLTransformerSS(task_mlm_itm_mpp(num_layers=2, per_gpu_batchsize=4, drop_rate=0.0, load_path=path, loss_names=_loss_names({"mpp": 1})),
                          device=DEV, compute_dtype="bf16")
    assert m2.load_report["missing"] == [] and m2.load_report["unexpected"] == []
    for k in M.HEAD:
        assert torch.equal(m2.state_dict()[k].cpu(), p[k]), k
    # a pixel outside [-1, 1] in a masked patch: a label outside 0..255 is a ValueError that names the pixel range
    b2 = with_masks(dev_batch(batch), masked, replaced)
    img = b2["image"][0].clone()
    q = int(masked[1].nonzero()[0])
    img[1, :, (q // 12) * 32:(q // 12) * 32 + 32, (q % 12) * 32:(q % 12) * 32 + 32] = 1.5
    b2["image"] = [img]
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        m.training_step(b2, 0)


def test_initialisation_and_optimizer_groups():
    torch.manual_seed(0)
    m = ViLTransformerSS(task_mlm_itm_mpp(num_layers=2, per_gpu_batchsize=2), device=DEV, compute_dtype="f32")
    sd = m.state_dict()
    assert torch.count_nonzero(sd["transformer.mask_token"]) == 0 and tuple(sd["transformer.mask_token"].shape) == (1, 1, 768)
    assert torch.equal(sd["mpp_score.transform.LayerNorm.weight"].cpu(), torch.ones(768))
    for n in ("mpp_score.transform.LayerNorm.bias", "mpp_score.transform.dense.bias", "mpp_score.decoder.bias"):
        assert torch.count_nonzero(sd[n]) == 0, n
    for n in ("mpp_score.transform.dense.weight", "mpp_score.decoder.weight"):
        assert abs(float(sd[n].std()) - 0.02) < 1e-3, n
    (opt,), _ = m.configure_optimizers()
    ends = opt.seg_end.cpu().tolist()
    for name, off, shape in m.engine.mpp_specs:
        i = next(j for j, e in enumerate(ends) if e > off)
        assert float(opt.seg_mult[i]) == 1.0, name
        decayed = name in ("transformer.mask_token", "mpp_score.transform.dense.weight", "mpp_score.decoder.weight")
        assert float(opt.seg_wd[i]) == pytest.approx(0.01 if decayed else 0.0), name
    for ln in ({"mpp": 1, "moco": 1}, {"mpp": 1, "barlowtwins": 1}):
        with pytest.raises(NotImplementedError):
            ViLTransformerSS(task_mlm_itm_mpp(num_layers=2, per_gpu_batchsize=2, loss_names=_loss_names(ln)), device=DEV, compute_dtype="f32")


def test_task_mlm_itm_mpp_trains_through_training_step_and_adamw_lowers_the_mpp_loss():
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=8)
    torch.manual_seed(3)
    m = ViLTransformerSS(task_mlm_itm_mpp(num_layers=2, per_gpu_batchsize=8, drop_rate=0.1, max_steps=100, warmup_steps=0), device=DEV,
                         compute_dtype="bf16")
    (opt,), _ = m.configure_optimizers()
    batch = ML.synthetic_mlm(O.synthetic_batch(cfg, 8, 5, ragged_text=True), 6, cfg["vocab_size"])
    masked, replaced = M.make_masks(batch["image"][0], cfg, 7, "random")
    db = with_masks(dev_batch(batch), masked, replaced)
    m.train()
    losses = []
    for it in range(20):
        m.zero_grad()
        loss = m.training_step(db, it)
        loss.backward()
        opt.step()
        losses.append(float(m.logged["mpp/train/loss"]))
    assert set(m.current_tasks) == {"itm", "mlm", "mpp"}
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert float(dict(m.named_parameters())["transformer.mask_token"].abs().max()) > 0          # the mask token moved off its zero start


def test_epoch_accuracy_accumulates_and_resets():
    g, cfg, p, batch, masked, replaced, _ = M.load_case("mpp_L2_B4_ragged")
    m = make_module(cfg, p, "f32")
    db = with_masks(dev_batch(batch), masked, replaced)
    for _ in range(2):
        _step(m, db)
    m.training_epoch_end()
    ep = m.last_epoch_metrics
    assert ep["mpp/train/accuracy_epoch"] == pytest.approx(int(g["correct"]) / (3 * int(g["n"])))
    assert "train" not in m.mpp_epoch_counts


def test_two_rank_step_keeps_the_ranks_bit_identical():
    """The N > 1 code path of the mlm + itm + mpp step: two ranks (gloo instead of RCCL, both on cuda:0) run tools/mpp_two_rank.py with
    different batches and masks per rank; the three deferred backwards share one gradient reduction and the parameters - the mask token
    and mpp_score included - must come out bit-identical on both ranks (the reference's DDP invariant)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29741", os.path.join(root, "tools", "mpp_two_rank.py"), "--steps", "2", "--batch", "4"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["world_size"] == 2 and rec["ranks_bit_identical"] is True
    assert rec["final_loss"] == rec["final_loss"] and rec["mask_token_abs_max"] > 0            # finite; the mask token took its steps
