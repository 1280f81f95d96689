"""-m gpu: ``rmcl_amd.Predictor.align`` end to end.

fp32 engine against the fixture tests/golden/align_L2.npz (tools/gen_golden_align.py: the reference's own model, cost_matrix_cosine, ipot
and the demo's heat arithmetic; tests/align_fixture.py).  dC = max |cost - cost_ref| is measured, printed and held to the budget the
generator's margins assume (align_fixture.DC_BUDGET).  After t iterations the plan behaves like exp(-t C / beta) rescaled, so entries
above 1e-3 max T may deviate by a relative 4 t dC / beta (one such term each from the numerator, delta and sigma, one for margin) plus
the kernel allowance of tests/test_align_kernels_gpu.py, 8 * max(e32, 2^-23 max T) with the e32 the generator stored.  For t = 50 and
t = 1000: the same flat positions, the same set of non-zero heat cells, the same arg-max cell, equal bytes wherever the generator stored
a margin, and for the chosen positions the alpha channel PIL's NEAREST resize made.  No case is skipped.

bf16 engine.  Its cost drifts from the reference's by about 1e-2, and t dC / beta is then about 100 at t = 1000: a 1000-step plan of
that engine is not comparable with the reference's.  What is pinned instead is the chain behind the encoder: the cost against the float64
cosine cost of the engine's OWN pb.xn, the plan against the float64 oracle on that cost, heat and bytes against the float64 model of that
plan - each under its kernel's allowance.

The measured numbers go, next to their bounds, to the file named by RMCL_ALIGN_PARITY_OUT when set (profiles/align_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd import Predictor  # noqa: E402
from rmcl_amd.vilt.config import task_moco  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from oracle import rmcl_oracle as O  # noqa: E402
from tests import align_fixture as AF  # noqa: E402
from tests import align_ref as R  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402
from tests.test_wpa_kernels_gpu import IPOT_FACTOR  # noqa: E402

DEV = "cuda:0"
OBSERVED = {}


@pytest.fixture(scope="module", autouse=True)
def parity_dump():
    yield
    out = os.environ.get("RMCL_ALIGN_PARITY_OUT")
    if out and OBSERVED:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec["predictor"] = {"what": "Predictor.align on tests/golden/align_L2.npz: dC = max |cost - cost_ref| (budget: the generator's), the largest "
                                    "relative plan deviation on entries above 1e-3 max T after the kernel allowance, next to 4 t dC / beta", **OBSERVED}
        with open(out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")


def make_module(dtype, drop_rate=0.0):
    cfg = task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=2, adv_steps_img=2, drop_rate=drop_rate, image_view=True)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype=dtype)
    p = O.init_params(AF.config(), AF.SEEDS["weights"])
    m.load_state_dict({n: t.to(DEV) for n, t in p.items()}, strict=False)
    return m


def engine_state(m):
    return ([mod.training for mod in m.modules()], m.engine.dropout_on, m.engine.pass_counter)


@pytest.mark.parametrize("case", list(AF.CASES))
def test_fp32_engine_reproduces_the_fixture(case):
    g = load(AF.FIXTURE)
    batch = AF.make_batch(AF.config(), case)
    m = make_module("f32")
    m.train()
    state = engine_state(m)
    pr = Predictor(m, tokenizer=AF.VOCAB)
    H, W = (int(v) for v in g[f"{case}_grid_hw"])
    B = batch["text_ids"].shape[0]
    token = g[f"{case}_token"].tolist()
    cells, cost_ref = g[f"{case}_cells"], g[f"{case}_cost"]
    for t in AF.ITERS:
        res = pr.align(batch["image"][0], text_ids=batch["text_ids"], text_masks=batch["text_masks"], token=token, iterations=t, beta=AF.BETA)
        assert engine_state(m) == state and torch.is_grad_enabled()
        assert res["grid_hw"] == (H, W) and tuple(res["heat"].shape) == (B, 40, H, W)
        dC = float(np.abs(res["cost"].cpu().numpy() - cost_ref).max())
        rel = AF.relative_bound(t, dC)
        ref, (e32, tmax) = g[f"{case}_plan_{t}"].astype(np.float64), g[f"{case}_e32_{t}"]
        kernel_allow = IPOT_FACTOR * max(e32, 2.0 ** -23 * tmax)
        plan = res["plan"].cpu().numpy().astype(np.float64)
        big = ref > 1e-3 * ref.max()
        excess = np.maximum(np.abs(plan - ref) - kernel_allow, 0.0)
        worst = float((excess[big] / ref[big]).max())
        print(f"align {case} t = {t}: dC {dC:.3e} (budget {AF.DC_BUDGET:.1e})  4 t dC / beta {rel:.3e}  largest relative plan deviation {worst:.3e}  "
              f"kernel allowance {kernel_allow:.3e}")
        OBSERVED[f"{case}_t{t}"] = {"dC": dC, "dC_budget": AF.DC_BUDGET, "relative_bound": rel, "largest_relative_plan_deviation": worst,
                                    "kernel_allowance": kernel_allow}
        assert dC <= AF.DC_BUDGET
        assert worst <= rel
        assert (plan[~big] <= (1 + rel) * 1e-3 * ref.max() + kernel_allow).all()
        assert (plan[ref == 0] == 0).all()                                                  # every joint pad of the reference's plan
        assert np.array_equal(res["grid"].cpu().numpy().view(np.int32), R.scatter(res["plan"].cpu().numpy(), cells, H, W).view(np.int32))
        heat, flat = res["heat"].cpu().numpy(), res["flat"].cpu().numpy()
        assert np.array_equal(flat, g[f"{case}_flat_{t}"])
        href, bref, ok = g[f"{case}_heat_{t}"], g[f"{case}_bytes_{t}"], g[f"{case}_byte_ok_{t}"]
        assert (heat[flat == 1] == 0).all()
        for b, mpos in zip(*np.nonzero(flat == 0)):
            assert np.array_equal(heat[b, mpos] > 0, href[b, mpos] > 0), (case, t, b, mpos)
            assert int(heat[b, mpos].argmax()) == int(href[b, mpos].argmax()), (case, t, b, mpos)
            assert np.array_equal(R.alpha_bytes(heat[b, mpos], H, W)[ok[b, mpos]], bref[b, mpos][ok[b, mpos]]), (case, t, b, mpos)
        alpha = res["alpha"].cpu().numpy()
        assert alpha.shape == (B,) + tuple(batch["image"][0].shape[2:]) and alpha.dtype == np.uint8      # default size: the bound batch's extent
        ty, tx = R.nearest_table(H, alpha.shape[1]), R.nearest_table(W, alpha.shape[2])
        for b in range(B):
            assert np.array_equal(alpha[b], R.alpha_bytes(heat[b, token[b]], *alpha.shape[1:]))
            if t == AF.ITERS[-1]:
                okb = ok[b, token[b]][ty][:, tx]
                assert okb.any() and np.array_equal(alpha[b][okb], g[f"{case}_alpha_{t}"][b][okb])
    words = pr.tokenizer.convert_ids_to_tokens(batch["text_ids"][0].tolist())
    assert res["tokens"][0] == words and res["tokens"][0][0] == "[CLS]" and len(res["tokens"]) == B
    small = pr.align(batch["image"][0], text_ids=batch["text_ids"], text_masks=batch["text_masks"], token=token[0], iterations=3, size=(5, 7))
    assert tuple(small["alpha"].shape) == (B, 5, 7)
    assert "alpha" not in pr.align(batch["image"][0], text_ids=batch["text_ids"], text_masks=batch["text_masks"], iterations=3)


def test_bf16_engine_against_the_float64_model_of_its_own_features():
    case = "ragged"
    batch = AF.make_batch(AF.config(), case)
    m = make_module("bf16")
    pr = Predictor(m)
    B, Lt = batch["text_ids"].shape
    for t in AF.ITERS:
        res = pr.align(batch["image"][0], text_ids=batch["text_ids"], text_masks=batch["text_masks"], token=[3, 2], iterations=t, beta=AF.BETA)
        pb = [v for k, v in m.engine._bufs.items() if k[1] == "predict"][-1]
        Li = pb.d.P + 1
        xn = pb.xn.double().cpu().view(B, Lt + Li, -1)
        tv, iv = AF.demo_masks(batch["text_masks"], pb.co_mask[:, Lt:].cpu())
        xh = torch.nn.functional.normalize(xn, dim=-1, eps=1e-5)
        jp = ~tv[:, :, None] | ~iv[:, None, :]
        c64 = (1 - xh[:, :Lt] @ xh[:, Lt:].transpose(1, 2)).masked_fill(jp, 0)
        cost = res["cost"].cpu()
        assert float((cost.double() - c64).abs().max()) <= 1e-5                             # the exact-f32 rule of tests/test_wpa_kernels_gpu.py
        assert (cost[jp] == 0).all()

        def oracle(dt):
            return O.ipot(cost.to(dt), tv.sum(1).to(dt), ~tv, iv.sum(1).to(dt), ~iv, jp, AF.BETA, t, 1)

        T64, T32 = oracle(torch.float64), oracle(torch.float32)
        base = max(float((T32.double() - T64).abs().max()), 2.0 ** -23 * float(T64.max()))
        dev = float((res["plan"].cpu().double() - T64).abs().max())
        OBSERVED[f"bf16_{case}_t{t}"] = {"plan_dev_over_base": dev / base, "allowed_ratio": IPOT_FACTOR}
        assert dev <= IPOT_FACTOR * base, (t, dev, base)
        H, W = res["grid_hw"]
        kept = torch.arange(pb.d.P)[None, :] < pb.geom.counts.cpu()[:, None]
        cells = torch.where(kept, pb.geom.sel[:, :pb.d.P].cpu(), torch.full((1,), -1, dtype=torch.int32)).numpy()
        plan = res["plan"].cpu().numpy()
        grid = R.scatter(plan, cells, H, W)
        assert np.array_equal(res["grid"].cpu().numpy().view(np.int32), grid.view(np.int32))
        heat64, flat64 = R.heat_model(grid.astype(np.float64), tv.numpy())
        heat = res["heat"].cpu().numpy()
        assert np.array_equal(res["flat"].cpu().numpy(), flat64) and (flat64 == 0).any()
        for b, mpos in zip(*np.nonzero(flat64 == 0)):
            assert np.abs(heat[b, mpos] - heat64[b, mpos]).max() <= R.heat_allowance(grid[b, mpos]), (t, b, mpos)
        alpha = res["alpha"].cpu().numpy()
        for b, tok in enumerate((3, 2)):
            assert np.array_equal(alpha[b], R.alpha_bytes(heat[b, tok], *alpha.shape[1:]))


def test_a_training_step_after_align_has_the_bits_of_the_step_without_it():
    ocfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=2, adv_steps_img=2)
    tb = O.synthetic_batch(ocfg, 2, 4)
    ab = AF.make_batch(AF.config(), "ragged")
    losses = []
    for align_first in (False, True):
        torch.manual_seed(3)
        m = make_module("bf16", drop_rate=0.1)
        m.proj_queue.copy_(O.init_queue(ocfg, 0).to(DEV))
        m.train()
        if align_first:
            Predictor(m).align(ab["image"][0], text_ids=ab["text_ids"], text_masks=ab["text_masks"], token=1, iterations=20)
            assert m.training and all(mod.training for mod in m.modules())
        loss = m.training_step(dev_batch(tb), 0)
        torch.cuda.synchronize()
        losses.append(loss.detach().clone())
    assert torch.isfinite(losses[0]) and torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32))


def test_align_refuses_bad_arguments():
    m = make_module("f32")
    pr = Predictor(m)
    b = AF.make_batch(AF.config(), "square")
    img, kw = b["image"][0], dict(text_ids=b["text_ids"], text_masks=b["text_masks"])
    for bad, word in ((dict(token=40), "0 .. 39"), (dict(token=-1), "0 .. 39"), (dict(token=[1, 2]), "one per sample"),
                      (dict(iterations=0), "1 .. 10000"), (dict(iterations=10001), "1 .. 10000"), (dict(beta=0.0), "beta must be > 0"),
                      (dict(beta=-1.0), "beta must be > 0"), (dict(token=1, size=(0, 5)), "size"), (dict(text="a b"), "either text")):
        with pytest.raises(ValueError, match=word):
            pr.align(img, **dict(kw, **bad))
    with pytest.raises(ValueError, match="tokenizer"):
        pr.align(img, text="a word")
    eng = m.engine
    plan = torch.zeros(1, 17, 40, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        eng.align_heat(plan, torch.zeros(1, 16, dtype=torch.int32, device=DEV), torch.ones(1, 40, dtype=torch.int32, device=DEV), (65, 64))
    with pytest.raises(ValueError, match="1 .. 10000"):
        eng.ipot_plan(torch.zeros(1, 40, 20, device=DEV), torch.ones(1, 40, dtype=torch.int32, device=DEV),
                      torch.ones(1, 17, dtype=torch.int32, device=DEV), 0.1, 20000)
