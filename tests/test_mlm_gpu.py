"""-m gpu: masked language modelling (task_mlm_itm) - the HIP kernels of csrc/mlm.hip against torch in fp64, the whole mlm and
mlm + itm steps against the reference's own run (tests/golden/mlm_*.npz from tools/gen_golden_mlm.py) and against the CPU oracle
(tests/mlm_oracle.py), plus the module-level contracts: state dict, infer(mask_text=True), the all-ignored batch, label validation.

Observed parity per fixture, quantity and dtype: profiles/mlm_parity.json (written by tools/mlm_parity.py from these same comparisons)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from oracle import rmcl_oracle as O  # noqa: E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P  # noqa: E402
from rmcl_amd.runtime import mlm_layout, stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_mlm_itm, task_moco, default_config, _loss_names  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from tests import mlm_oracle as M  # noqa: E402
from tests.golden_util import digest  # noqa: E402
from tests.test_path_gpu import dev_batch  # noqa: E402

DEV = "cuda:0"
C = L.C
F = C.c_float
HEAD = [n for n, _ in M.mlm_param_shapes({"hidden_size": 768, "vocab_size": 30522})]
D = 768


# ---- kernels ------------------------------------------------------------------------------------------------------------
def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _kernel_case(n, V, seed, tie=False, D=D):
    """n labelled positions among B x 40 text positions of an xn with 46 token rows per sample; a head with peaked logits."""
    Lt, N = 40, 46
    B = max(2, -(-n // Lt))
    cfg = {"hidden_size": D, "vocab_size": V}
    h, specs, total = mlm_layout(cfg, 0)
    g = torch.Generator().manual_seed(seed)
    arena = torch.zeros(total)
    w = {}
    for name, off, shape in specs:
        if name.endswith("LayerNorm.weight"):
            t = 1 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("decoder.weight"):
            t = 4.0 * torch.randn(shape, generator=g) / D ** 0.5
        elif len(shape) == 2:
            t = torch.randn(shape, generator=g) / D ** 0.5
        else:
            t = 0.3 * torch.randn(shape, generator=g)
        if tie and name.endswith("decoder.weight"):
            t[V - 3] = t[5]                                  # two identical columns far apart (different tiles, chunks and lanes) ...
        if tie and name == "mlm_score.bias":
            t[5] = t[V - 3] = 30.0                           # ... that win every row: the FIRST maximum is column 5
        arena[off:off + t.numel()] = t.flatten()
        w[name] = t
    xn = torch.randn(B * N, D, generator=g)
    labels = torch.full((B * Lt,), -100, dtype=torch.int64)
    pos = torch.randperm(B * Lt, generator=g)[:n].sort().values
    labels[pos] = torch.randint(0, V, (n,), generator=g)
    if n >= 2:
        labels[pos[1]] = labels[pos[0]]                      # one label in two rows
    return h, specs, arena, w, xn, labels.view(B, Lt), N


def _run_kernels(h, arena, xn, labels, N, dtype, gscale=1.0, want_logits=True, with_dxn=True):
    B, Lt = labels.shape
    Mt = B * Lt
    n = int((labels != -100).sum())
    rows = max(128, (n + 127) // 128 * 128)
    dt = L.BF16 if dtype == "bf16" else L.F32
    a = arena.to(DEV)
    lp = a.to(torch.bfloat16) if dt == L.BF16 else None
    i32 = lambda k: torch.full((k,), -7, dtype=torch.int32, device=DEV)
    f32 = lambda k: torch.full((k,), float("nan"), dtype=torch.float32, device=DEV)
    idx, lab, cnt = i32(Mt), i32(Mt), i32(1)
    lse, rl, am, stats = f32(rows), f32(rows), i32(rows), f32(3)
    ws = torch.empty(int(lib.rmcl_mlm_ws_floats(C.byref(h), rows)), device=DEV)
    ldv = (h.V + 127) // 128 * 128
    wT = torch.empty(h.D, ldv, dtype=torch.bfloat16 if dt == L.BF16 else torch.float32, device=DEV)
    G = torch.zeros_like(a)
    dxn = torch.zeros(xn.shape, device=DEV) if with_dxn else None
    x, lb = xn.to(DEV), labels.to(DEV).contiguous()
    gs = torch.tensor([gscale], device=DEV)
    check(lib.rmcl_mlm_compact(P(lb), Mt, Lt, N, h.V, 0, P(idx), P(lab), P(cnt), stream_ptr()))
    check(lib.rmcl_mlm_weight_transpose(C.byref(h), P(a), P(wT), dt, stream_ptr()))
    check(lib.rmcl_mlm_forward(C.byref(h), P(a), P(lp), dt, P(x), P(idx), P(lab), P(cnt), rows, P(ws), P(lse), P(rl), P(am), P(stats), stream_ptr()))
    check(lib.rmcl_mlm_backward(C.byref(h), P(a), P(lp), P(wT), dt, P(idx), P(lab), P(cnt), rows, P(ws), P(lse), F(1.0), P(gs), P(G), P(dxn),
                                stream_ptr()))
    logits = None
    if want_logits and n:
        logits = torch.empty(n, h.V, device=DEV)
        check(lib.rmcl_mlm_logits(C.byref(h), P(a), P(lp), dt, P(ws), rows, n, P(logits), L.I64(h.V), stream_ptr()))
    torch.cuda.synchronize()
    return dict(idx=idx, lab=lab, cnt=cnt, lse=lse, rowloss=rl, argmax=am, stats=stats, G=G, dxn=dxn, logits=logits, n=n, rows=rows)


def _fp64_reference(h, specs, w, xn, labels, N, dtype, gscale):
    """The head in fp64 with autograd.  bf16 engine: the decoder's operands are what the kernels multiply - the bf16 shadow of
    decoder.weight and h rounded to bf16 (straight-through for the gradient) - so the comparison measures the kernels' arithmetic
    (fp32 accumulation, fp32 softmax), not the operand rounding that the golden tests bound."""
    wd = {k: v.double().requires_grad_(True) for k, v in w.items()}
    x0 = xn.double().requires_grad_(True)
    rows_i, lab, n = M.compact(labels, N)
    x = x0[torch.from_numpy(rows_i)]
    hh = M.mlm_transform(wd, x)
    Wd = wd["mlm_score.decoder.weight"]
    if dtype == "bf16":
        hh = hh + (bf16_round(hh.detach().float()).double() - hh.detach())
        Wd = Wd + (bf16_round(Wd.detach().float()).double() - Wd.detach())
    z = hh @ Wd.t() + wd["mlm_score.bias"]
    labt = torch.from_numpy(lab)
    rl = torch.nn.functional.cross_entropy(z, labt, reduction="none")
    (gscale * rl.sum() / n).backward()
    return dict(z=z.detach(), rowloss=rl.detach(), lse=torch.logsumexp(z.detach(), 1), w=wd, x0=x0, rows_i=rows_i, lab=labt, n=n)


# kernel tolerances, from the number formats (not from the kernels' output): fp32 engine - fp32 products and sums over K = 768 against
# fp64, the bound of the VQA kernel test (1e-4 on logits, 2e-4 on gradients).  bf16 engine - the reference multiplies the same bf16
# operands, so what is left is (a) fp32 accumulation and (b) an occasional element of h whose fp32 value rounds to the other bf16
# neighbour than the fp64 value does: one such flip moves a logit by |h_i| 2^-8 |W_vi| ~ 1e-3, a handful per row 5e-3; the
# recomputed dz is rounded to bf16 (2^-9 relative per term, random signs) before the dW / dh products and the dbias sums: 2e-2 of a
# tensor's maximum covers sqrt(rows) such terms with a wide margin.
KTOL = {"f32": dict(z=1e-4, loss=1e-5, grad=2e-4), "bf16": dict(z=5e-3, loss=2e-3, grad=2e-2)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
# hidden 256 is the other width the launcher takes: one float4 per lane in the transform's row pass (768 has three), two k-tiles per z tile
@pytest.mark.parametrize("n,V,Dh", [pytest.param(1, 30522, 768, id="1-30522"), pytest.param(37, 30522, 768, id="37-30522"),
                                    pytest.param(384, 30522, 768, id="384-30522"), pytest.param(2560, 30522, 768, id="2560-30522"),
                                    pytest.param(37, 1000, 768, id="37-1000"), pytest.param(384, 1000, 768, id="384-1000"),
                                    pytest.param(1, 1000, 768, id="1-1000"), pytest.param(1, 1000, 256, id="1-1000-D256"),
                                    pytest.param(37, 1000, 256, id="37-1000-D256")])
def test_mlm_kernels_match_torch_fp64(n, V, Dh, dtype):
    h, specs, arena, w, xn, labels, N = _kernel_case(n, V, 1000 + n + V + (0 if Dh == 768 else Dh), D=Dh)
    r = _run_kernels(h, arena, xn, labels, N, dtype, gscale=0.5)
    ref = _fp64_reference(h, specs, w, xn, labels, N, dtype, 0.5)
    tol = KTOL[dtype]
    assert int(r["cnt"]) == n == ref["n"]
    # compaction: ascending rows, their labels; -1 / -100 behind the count
    assert torch.equal(r["idx"][:n].cpu().long(), torch.from_numpy(ref["rows_i"]))
    assert torch.equal(r["lab"][:n].cpu().long(), ref["lab"])
    assert bool((r["idx"][n:] == -1).all()) and bool((r["lab"][n:] == -100).all())
    zmax = max(1.0, float(ref["z"].abs().max()))
    z = r["logits"].cpu().double()
    ez = float((z - ref["z"]).abs().max())
    el = float((r["lse"][:n].cpu().double() - ref["lse"]).abs().max())
    er = float((r["rowloss"][:n].cpu().double() - ref["rowloss"]).abs().max())
    print(f"mlm kernels n={n} V={V} {dtype}: |dz|max {ez:.3e} lse {el:.3e} rowloss {er:.3e} (|z|max {zmax:.2f})")
    assert ez < tol["z"] * zmax
    assert el < tol["z"] * zmax and er < 2 * tol["z"] * zmax
    # rows behind the count contribute nothing
    assert bool((r["rowloss"][n:] == 0).all()) and bool((r["argmax"][n:] == -1).all())
    # argmax: the reference's wherever its top-two gap is clear of the logits tolerance
    top2 = ref["z"].topk(2, dim=1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * tol["z"] * zmax
    am = r["argmax"][:n].cpu().long()
    assert bool(((am >= 0) & (am < V)).all())
    assert torch.equal(am[clear], top2.indices[:, 0][clear])
    # the argmax the kernel reports is the first maximum of the logits the kernels themselves write
    assert torch.equal(am, r["logits"].argmax(dim=1).cpu())
    # stats = (mean row loss, correct rows, n)
    st = r["stats"].cpu().double()
    assert abs(float(st[0]) - float(ref["rowloss"].mean())) < tol["loss"] * float(ref["rowloss"].mean())
    assert float(st[1]) == float((am == ref["lab"]).sum()) and float(st[2]) == n
    # gradients: every head tensor, and the scattered data gradient (zero outside the labelled rows)
    for name, off, shape in specs:
        got = r["G"][off:off + w[name].numel()].view(shape).cpu().double()
        want = ref["w"][name].grad
        err = float((got - want).abs().max())
        print(f"   grad {name}: {err:.3e} of {float(want.abs().max()):.3e}")
        assert err < tol["grad"] * float(want.abs().max()) + 1e-12, name
    gx = ref["x0"].grad
    assert float((r["dxn"].cpu().double() - gx).abs().max()) < tol["grad"] * float(gx.abs().max())
    other = torch.ones(xn.shape[0], dtype=torch.bool)
    other[torch.from_numpy(ref["rows_i"])] = False
    assert torch.count_nonzero(r["dxn"].cpu()[other]) == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_argmax_ties_go_to_the_first_column(dtype):
    h, specs, arena, w, xn, labels, N = _kernel_case(37, 30522, 5, tie=True)
    r = _run_kernels(h, arena, xn, labels, N, dtype)
    lg = r["logits"]
    assert torch.equal(lg[:, 5], lg[:, 30522 - 3])                         # identical operands: identical bits in both columns
    assert bool((r["argmax"][:37] == 5).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mlm_kernels_are_bit_reproducible(dtype):
    h, specs, arena, w, xn, labels, N = _kernel_case(384, 30522, 9)
    a = _run_kernels(h, arena, xn, labels, N, dtype)
    b = _run_kernels(h, arena, xn, labels, N, dtype)
    for k in ("idx", "lab", "cnt", "lse", "rowloss", "argmax", "stats", "G", "dxn", "logits"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_all_ignored_batch_kernels(dtype):
    """n = 0: NaN loss like F.cross_entropy over an all-ignored batch, nothing but zeros added to the gradient arena, no NaN in dxn."""
    h, specs, arena, w, xn, labels, N = _kernel_case(0, 1000, 3)
    r = _run_kernels(h, arena, xn, labels, N, dtype)
    assert int(r["cnt"]) == 0 and bool(torch.isnan(r["stats"][0])) and float(r["stats"][2]) == 0
    assert torch.count_nonzero(r["G"]) == 0 and torch.count_nonzero(r["dxn"]) == 0
    assert bool(torch.isfinite(r["G"]).all()) and bool(torch.isfinite(r["dxn"]).all())


def test_backward_without_dxn_leaves_the_same_gradient_arena():
    """dxn = NULL: the transform backward launches neither the dx = da Wt GEMM nor the scatter (nobody reads dx), and every head
    gradient holds the bits of a call with dxn.  The module's smallest case: one labelled row, rows = 128, V = 1000, D = 256."""
    h, specs, arena, w, xn, labels, N = _kernel_case(1, 1000, 1000 + 1 + 1000 + 256, D=256)
    for dtype in ("f32", "bf16"):
        a = _run_kernels(h, arena, xn, labels, N, dtype, want_logits=False)
        b = _run_kernels(h, arena, xn, labels, N, dtype, want_logits=False, with_dxn=False)
        assert a["rows"] == 128 and b["dxn"] is None and torch.count_nonzero(a["dxn"]) > 0
        for name, off, shape in specs:
            sl = slice(off, off + w[name].numel())
            assert torch.count_nonzero(a["G"][sl]) > 0, name
        assert torch.equal(a["G"], b["G"]), dtype


# ---- module -------------------------------------------------------------------------------------------------------------
def make_mlm_module(ocfg, p, dtype="f32", with_itm=False, with_mlm=True, **over):
    kw = dict(num_layers=ocfg["num_layers"], per_gpu_batchsize=ocfg["per_gpu_batchsize"], drop_rate=0.0, max_steps=100, warmup_steps=0,
              loss_names=_loss_names({"mlm": int(with_mlm), "itm": int(with_itm)}))
    kw.update(over)
    m = ViLTransformerSS(task_mlm_itm(**kw), device=DEV, compute_dtype=dtype)
    skip = ("k_", "moco_head") + (() if with_itm else ("itm_score",)) + (() if with_mlm else ("mlm_score",))
    sd = {n: t.to(DEV) for n, t in p.items() if not n.startswith(skip)}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    m.train()
    return m


def _step(m, batch):
    m.zero_grad()
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    return loss


# TOL of tests/test_vqa_gpu.py: fp32 engine - the repository's fp32 contract; bf16 engine - the bf16 class of the golden tests
TOL = {"f32": dict(loss=1e-3, logits=2e-3, grad=2e-3), "bf16": dict(loss=1e-2, logits=0.1, grad=0.1)}


def compare_with_golden(name, dtype):
    """Runs one fixture and returns (observed errors, failures): shared by the test below and tools/mlm_parity.py."""
    g, cfg, p, batch, with_itm = M.load_case(name)
    tol = TOL[dtype]
    m = make_mlm_module(cfg, p, dtype, with_itm)
    if with_itm:
        m.itm_labels_override = torch.from_numpy(g["itm_labels"])
    db = dev_batch(batch)
    loss = _step(m, db)
    obs, bad = {}, []

    def chk(key, err, bound):
        obs[key] = float(err)
        if not err <= bound:
            bad.append((key, float(err), float(bound)))

    B, n = cfg["per_gpu_batchsize"], int(g["n"])
    eng = m.engine
    mb = eng.mlm_bufs(B, "mlm")
    stats_n = int(mb.count)
    assert stats_n == n
    mlm_loss = float(m.logged["mlm/train/loss"])
    if n == 0:
        assert np.isnan(float(g["mlm_loss"])) and np.isnan(mlm_loss) and np.isnan(float(loss))
    else:
        ref_total = float(g["total_loss"]) if with_itm else float(g["mlm_loss"])
        chk("loss_rel", abs(float(loss) - ref_total) / ref_total, tol["loss"])
        chk("mlm_loss_rel", abs(mlm_loss - float(g["mlm_loss"])) / float(g["mlm_loss"]), tol["loss"])
        zmax = max(1.0, float(g["zmax"]))
        rl = mb.rowloss[:n].cpu().numpy()
        chk("row_loss_abs_over_max", np.abs(rl - g["row_loss"]).max() / max(1.0, np.abs(g["row_loss"]).max()), tol["loss"])
        lg = eng.mlm_logits(mb, n)[:, torch.from_numpy(g["sample_cols"]).to(DEV)].cpu().numpy()
        chk("logits_abs_over_zmax", np.abs(lg - g["sample_logits"]).max() / zmax, tol["logits"])
        # argmax / accuracy: integers, exact in f32.  bf16: a row may differ only where the REFERENCE's top-two gap is below the logits
        # tolerance; such rows are counted apart and may be at most 2 % of the masked rows (the generator asserts the reference has none)
        am = mb.argmax[:n].cpu().numpy()
        differ = am != g["argmax"]
        near = g["gap"] < tol["logits"] * zmax
        obs["argmax_differ"] = int(differ.sum())
        obs["near_tie_rows"] = int(near.sum())
        if dtype == "f32":
            assert not differ.any() and int(round(float(m.logged["mlm/train/accuracy"]) * n)) == int(g["correct"])
            assert abs(float(m.logged["mlm/train/accuracy"]) - float(g["log_accuracy"])) < 1e-6
        else:
            assert not (differ & ~near).any(), ("argmax differs on a row with a clear gap", np.flatnonzero(differ & ~near))
            assert near.sum() <= 0.02 * n
    if with_itm:
        chk("itm_loss_rel", abs(float(m.logged["itm/train/loss"]) - float(g["itm_loss"])) / float(g["itm_loss"]), tol["loss"])
    params = dict(m.named_parameters())
    worst = 0.0
    for nm, d in zip(g["grad_names"], g["grad_digest"]):
        got = digest(params[str(nm)].grad)
        if n == 0 and str(nm).startswith("mlm_score"):
            assert d[1] == 0 and got[1] == 0, str(nm)                       # the all-zero gradient of the all-ignored batch
            continue
        if n == 0:
            assert np.isfinite(got).all() and got[1] == 0, str(nm)
            continue
        e = abs(got[1] - d[1]) / (d[1] + 1e-30)
        worst = max(worst, e)
        if not abs(got[1] - d[1]) <= tol["grad"] * d[1] + 1e-7:
            bad.append(("grad_digest " + str(nm), float(e), tol["grad"]))
    obs["grad_digest_l2_rel_worst"] = worst
    if n:
        cols = torch.from_numpy(g["sample_cols"]).to(DEV)
        wr = torch.from_numpy(g["word_rows"]).to(DEV)
        slices = (("grad_decoder_w", params[HEAD[5]].grad[cols[:16], :64]), ("grad_mlm_bias", params[HEAD[0]].grad[cols]),
                  ("grad_dense_w", params[HEAD[1]].grad[:8, :64]), ("grad_dense_b", params[HEAD[2]].grad[:64]),
                  ("grad_ln_w", params[HEAD[3]].grad[:64]), ("grad_ln_b", params[HEAD[4]].grad[:64]),
                  ("grad_word", params["text_embeddings.word_embeddings.weight"].grad[wr, :64]),
                  ("grad_qkv0_w", params["transformer.blocks.0.attn.qkv.weight"].grad[:8, :64]))
        for key, got in slices:
            ref = g[key]
            chk(key + "_abs_over_max", np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max(), tol["grad"] * 2.5)
    return obs, bad, m, db, g, cfg


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", M.FIXTURES)
def test_mlm_step_matches_reference_golden(name, dtype):
    obs, bad, m, db, g, cfg = compare_with_golden(name, dtype)
    print(name, dtype, obs)
    assert not bad, bad
    # the returned dict: the reference's keys; dense logits under no_grad in eval mode, and they agree with the fused statistics
    B, n = cfg["per_gpu_batchsize"], int(g["n"])
    out_train = m(db)
    assert set(("mlm_loss", "mlm_logits", "mlm_labels", "mlm_ids")) <= set(out_train) and out_train["mlm_logits"] is None
    assert out_train["mlm_labels"] is db["text_labels_mlm"] and out_train["mlm_ids"] is db["text_ids_mlm"]
    m.eval()
    with torch.no_grad():
        out = m(db)
    lg = out["mlm_logits"]
    assert lg.shape == (B, cfg["max_text_len"], cfg["vocab_size"])
    if n:
        on = db["text_labels_mlm"] != -100
        mb = m.engine.mlm_bufs(B, "mlm")
        rows = lg[on]
        assert torch.equal(rows.argmax(dim=1).to(torch.int32), mb.argmax[:n])
        assert float((torch.logsumexp(rows.double(), 1) - mb.lse[:n].double()).abs().max()) < 1e-4 * max(1.0, float(g["zmax"]))
        ref_loss = torch.nn.functional.cross_entropy(rows.double(), db["text_labels_mlm"][on])
        assert abs(float(out["mlm_loss"]) - float(ref_loss)) < 1e-5 * float(ref_loss)


def test_mlm_plus_itm_gradients_are_the_sum_of_the_single_task_gradients():
    """drop_rate = 0, ITM labels fixed: the two deferred backwards accumulate into the one arena (fp32 accumulation order only)."""
    g, cfg, p, batch, with_itm = M.load_case("mlm_itm_L2_B4")
    lab = torch.from_numpy(g["itm_labels"])
    grads = {}
    for key, (wm, wi) in (("both", (True, True)), ("mlm", (True, False)), ("itm", (False, True))):
        m = make_mlm_module(cfg, p, "f32", with_itm=wi, with_mlm=wm)
        m.itm_labels_override = lab
        _step(m, dev_batch(batch))
        grads[key] = {n_: prm.grad.clone() for n_, prm in m.named_parameters() if prm.grad is not None}
        del m
    for n_, gb in grads["both"].items():
        parts = [grads[k][n_] for k in ("mlm", "itm") if n_ in grads[k]]
        want = sum(parts)
        err = float((gb - want).abs().max())
        assert err <= 1e-6 * float(want.abs().max()) + 1e-30, (n_, err, float(want.abs().max()))


def test_mlm_bs64_bf16_matches_oracle():
    """The benchmarked shape (12 layers, bs = 64, bf16) against the CPU oracle with the same weights and batch, fresh seeds."""
    cfg = O.default_config(num_layers=12, per_gpu_batchsize=64)
    p = dict(O.init_params(cfg, 15), **M.mlm_init_params(cfg, 16))
    batch = M.synthetic_mlm(O.synthetic_batch(cfg, 64, 17, ragged_text=True), 18, cfg["vocab_size"])
    m = make_mlm_module(cfg, p, "bf16")
    loss = _step(m, dev_batch(batch))
    torch.set_num_threads(16)
    with torch.no_grad():
        r = M.compute_mlm(p, cfg, batch)
    print("bs64 bf16: hip", float(loss), "oracle", float(r["mlm_loss"]), "n", r["n"])
    assert int(m.engine.mlm_bufs(64, "mlm").count) == r["n"]
    assert abs(float(loss) - float(r["mlm_loss"])) < 1e-2 * float(r["mlm_loss"])
    params = dict(m.named_parameters())
    for n_ in HEAD:
        assert torch.isfinite(params[n_].grad).all() and float(params[n_].grad.abs().max()) > 0, n_


def test_state_dict_with_mlm_score_loads_and_round_trips(tmp_path):
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=2)
    p = dict(O.init_params(cfg, 1), **M.mlm_init_params(cfg, 2))
    sd = {n: t for n, t in p.items() if not n.startswith(("k_", "moco_head"))}
    path = str(tmp_path / "mlm_itm.ckpt")
    torch.save({"state_dict": sd}, path)
    m = ViLTransformerSS(task_mlm_itm(num_layers=2, per_gpu_batchsize=2, drop_rate=0.0, load_path=path), device=DEV, compute_dtype="f32")
    assert m.load_report["missing"] == [] and m.load_report["unexpected"] == []
    msd = m.state_dict()
    for n in HEAD:
        assert torch.equal(msd[n].cpu(), sd[n]), n
    m2 = ViLTransformerSS(default_config(num_layers=2, per_gpu_batchsize=2), device=DEV, compute_dtype="bf16")     # the package default: mlm + itm
    missing, unexpected = m2.load_state_dict(msd, strict=True)
    assert not missing and not unexpected
    for n in HEAD:
        assert torch.equal(m2.state_dict()[n], msd[n]), n


def test_moco_model_is_unchanged_by_the_mlm_head():
    m = ViLTransformerSS(task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=2, image_view=True), device=DEV, compute_dtype="f32")
    eng = m.engine
    assert eng.mlm is None and not eng.mlm_specs
    assert eng.total == int(eng.layout.total) and eng.q32.numel() == eng.g32.numel() == int(eng.layout.total)
    assert not any("mlm" in k for k in m.state_dict())


def test_head_initialisation():
    torch.manual_seed(0)
    m = ViLTransformerSS(task_mlm_itm(num_layers=2, per_gpu_batchsize=2), device=DEV, compute_dtype="f32")
    sd = m.state_dict()
    assert torch.equal(sd["mlm_score.transform.LayerNorm.weight"].cpu(), torch.ones(D))
    for n in ("mlm_score.transform.LayerNorm.bias", "mlm_score.transform.dense.bias", "mlm_score.bias"):
        assert torch.count_nonzero(sd[n]) == 0, n
    for n in ("mlm_score.transform.dense.weight", "mlm_score.decoder.weight"):
        assert abs(float(sd[n].std()) - 0.02) < 1e-3, n
    (opt,), _ = m.configure_optimizers()
    ends = opt.seg_end.cpu().tolist()
    for name, off, shape in m.engine.mlm_specs:
        i = next(j for j, e in enumerate(ends) if e > off)
        decay, head = O.param_group(name)
        assert not head and float(opt.seg_mult[i]) == 1.0, name                     # mlm_score is not in head_names: base learning rate
        assert float(opt.seg_wd[i]) == pytest.approx(0.01 if decay else 0.0), name
        assert decay == name.endswith(("dense.weight", "decoder.weight")), name      # bias / LayerNorm.* undecayed


def test_infer_mask_text_reads_the_mlm_ids():
    g, cfg, p, batch, _ = M.load_case("mlm_L2_B4_ragged")
    m = make_mlm_module(cfg, p, "f32")
    db = dev_batch(batch)
    with torch.no_grad():
        out = m.infer(db, mask_text=True)
        r = O.infer(p, cfg, batch["text_ids_mlm"], batch["text_masks"], batch["image"][0])
    assert out["text_ids"] is db["text_ids_mlm"] and out["text_labels"] is db["text_labels_mlm"]
    assert float((out["text_feats"].cpu() - r["text_feats"]).abs().max()) < 2e-3 * max(1.0, float(r["text_feats"].abs().max()))
    plain = m.infer(db)                                              # differentiable like infer is today
    assert plain["text_ids"] is db["text_ids"] and plain["text_labels"] is db["text_labels"]
    outg = m.infer(db, mask_text=True)
    outg["text_feats"].sum().backward()
    assert float(dict(m.named_parameters())["text_embeddings.word_embeddings.weight"].grad.abs().max()) > 0
    with pytest.raises(NotImplementedError):
        m.infer(db, mask_image=True)
    with pytest.raises(NotImplementedError):
        m.infer(db, mask_text=True, mask_image=True)


def test_label_outside_the_vocabulary_is_a_value_error():
    g, cfg, p, batch, _ = M.load_case("mlm_L2_B4_ragged")
    m = make_mlm_module(cfg, p, "f32")
    for bad in (cfg["vocab_size"], -1, -101):
        b2 = dict(batch)
        b2["text_labels_mlm"] = batch["text_labels_mlm"].clone()
        b2["text_labels_mlm"][1, 5] = bad
        with pytest.raises(ValueError):
            m.training_step(dev_batch(b2), 0)
        with pytest.raises(ValueError):
            m.training_step(b2 | {k: v for k, v in dev_batch(b2).items() if k != "text_labels_mlm"}, 0)      # labels still on the host


def test_epoch_accuracy_accumulates_and_resets():
    g, cfg, p, batch, _ = M.load_case("mlm_L2_B4_ragged")
    m = make_mlm_module(cfg, p, "f32")
    db = dev_batch(batch)
    for _ in range(2):
        _step(m, db)
    m.training_epoch_end()
    ep = m.last_epoch_metrics
    assert ep["mlm/train/accuracy_epoch"] == pytest.approx(int(g["correct"]) / int(g["n"]))
    assert "train" not in m.mlm_epoch_counts


def test_adamw_loop_with_dropout_lowers_the_loss():
    cfg = O.default_config(num_layers=2, per_gpu_batchsize=8)
    m = ViLTransformerSS(task_mlm_itm(num_layers=2, per_gpu_batchsize=8, drop_rate=0.1, max_steps=100, warmup_steps=0,
                                      loss_names=_loss_names({"mlm": 1})), device=DEV, compute_dtype="bf16")
    (opt,), _ = m.configure_optimizers()
    batch = dev_batch(M.synthetic_mlm(O.synthetic_batch(cfg, 8, 5, ragged_text=True), 6, cfg["vocab_size"]))
    m.train()
    losses = []
    for it in range(30):
        m.zero_grad()
        loss = m.training_step(batch, it)
        loss.backward()
        opt.step()
        losses.append(float(m.logged["mlm/train/loss"]))
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses
