"""-m gpu: the residual-through-LDS form of the 192x192 tile kernel (gemm_st.hip, rmcl_tune_set key 14) against the register form it
replaces where every workgroup has one tile.  The arithmetic of the two forms is the same operations on the same values in the same
order, so every comparison here is of RAW BITS: fp32 output, bf16 copy and row partials.  Each launch runs three times under key 14 = 1
and the three results must be identical - a race in the form's wait / barrier placement shows as a difference between repeats.
Output buffers carry a sentinel and guard rows behind M: rows no form may write are compared (and checked) too."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, I64, F, stream  # noqa: E402

EPI_BIAS, EPI_RESIDUAL, EPI_DROPOUT = 1, 8, 512
MS = [1, 97, 185, 192, 193, 370]      # one partial tile; both wave groups partly dead; rows_per_tile; the exact tile; two row tiles, uneven
NS = [192, 768]
KS = [128, 192, 768]                  # no steady-state k-tile at all; exactly one; the step's proj shape
M_MAX, GUARD = 370, 4


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def data():
    """Seeded operands, made once at the largest shape; a case takes the leading rows / columns."""
    return {"A": rnd(M_MAX, 768, seed=1).to(torch.bfloat16), "W": rnd(768, 768, seed=2, scale=0.05).to(torch.bfloat16), "b": rnd(768, seed=3),
            "R": rnd(M_MAX, 768 + 64, seed=4, scale=2.0), "c": rnd(M_MAX, seed=5, scale=3.0)}


class Tune:
    """rmcl_tune_set keys around a region (process-global: restored on the way out).  Key 0 = 60 asks for the 192x192 tile kernel."""
    DEFAULT = {0: -1, 1: 8, 14: 1}

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            check(lib.rmcl_tune_set(k, v), "tune_set")

    def __exit__(self, *exc):
        for k in self.kv:
            check(lib.rmcl_tune_set(k, self.DEFAULT[k]), "tune_set")


def operands(data, M, N, K):
    return data["A"][:M, :K].contiguous(), data["W"][:N, :K].contiguous(), data["b"][:N].contiguous()


def sentinel(M, N, dtype=torch.float32, fill=7.0):
    return torch.full((M + GUARD, N), fill, dtype=dtype, device=DEV)


def run_gemm(data, M, N, K, epi=EPI_BIAS | EPI_RESIDUAL, ld_aux=None, alias=False):
    """rmcl_gemm, fp32 output + fp32 residual (the FULL-pass producer).  alias: the residual IS the output buffer."""
    A, W, b = operands(data, M, N, K)
    ld_aux = N if ld_aux is None else ld_aux
    out = sentinel(M, N)
    if alias:
        out[:M] = data["R"][:M, :N]
        aux = out
    else:
        aux = data["R"][:M, :ld_aux].contiguous()
    assert lib.rmcl_gemm_route(M, N, K, epi, L.F32, 1, 1) == 1
    check(lib.rmcl_gemm(P(A), P(W), P(out), None, P(b), P(aux), M, N, K, I64(K), I64(K), N, ld_aux, F(1.0), epi, 1, L.BF16, L.F32, 1, 1, 0, stream()),
          "gemm")
    return (out,)


def run_rowstat(data, M, N, K, centred=False):
    """rmcl_linear_rowstat(_c): fp32 output, bf16 copy and row partials (the folded passes' producer)."""
    A, W, b = operands(data, M, N, K)
    R = data["R"][:M, :N].contiguous()
    out, outb = sentinel(M, N), sentinel(M, N, torch.bfloat16)
    part = torch.full((M + GUARD, 4 * (N // 192), 2), 7.0, device=DEV)
    if centred:
        cen = data["c"][:M].contiguous()
        check(lib.rmcl_linear_rowstat_c(P(A), P(W), P(b), P(R), P(cen), P(out), P(outb), P(part), M, N, K, stream()), "linear_rowstat_c")
    else:
        check(lib.rmcl_linear_rowstat(P(A), P(W), P(b), P(R), P(out), P(outb), P(part), M, N, K, stream()), "linear_rowstat")
    return out, outb, part


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(xs, ys, what):
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert torch.equal(bits(x), bits(y)), (what, i, int((bits(x) != bits(y)).sum()))


def guards_intact(outs, M):
    for o in outs:
        assert bool((o[M:].float() == 7.0).all())


def ab(run, what, M, **tune):
    """Three runs of the new form, one of the register form: all four bit-identical; guard rows untouched."""
    with Tune(k0=60, k14=1, **tune):
        new = [run() for _ in range(3)]
    with Tune(k0=60, k14=0, **tune):
        old = run()
    torch.cuda.synchronize()
    for r in new[1:]:
        same_bits(new[0], r, what + " repeat")
    same_bits(new[0], old, what)
    guards_intact(new[0], M)
    return new[0]


@pytest.mark.parametrize("M", MS)
def test_full_pass_producer_bits(data, M):
    for N in NS:
        for K in KS:
            ab(lambda: run_gemm(data, M, N, K), f"gemm M={M} N={N} K={K}", M)


@pytest.mark.parametrize("M", MS)
def test_rowstat_producer_bits(data, M):
    for N in NS:
        for K in KS:
            out, outb, part = ab(lambda: run_rowstat(data, M, N, K), f"rowstat M={M} N={N} K={K}", M)
            # written, not the sentinels of both forms (at N = 192 the exact kernels once took the launch and dropped the producer's outputs)
            assert torch.equal(outb[:M], out[:M].to(torch.bfloat16)) and not bool((part[:M] == 7.0).all()), (N, K)


@pytest.mark.parametrize("M", [1, 185, 193])
def test_centred_rowstat_producer_bits(data, M):
    ab(lambda: run_rowstat(data, M, 768, 192, centred=True), f"rowstat_c M={M}", M)


def test_strided_residual_bits(data):
    ab(lambda: run_gemm(data, 193, 768, 192, ld_aux=768 + 64), "gemm ld_aux = N + 64", 193)


def test_residual_aliasing_the_output_bits(data):
    out, = ab(lambda: run_gemm(data, 370, 768, 192, alias=True), "gemm aux == C", 370)
    with Tune(k0=60):                                         # in place = out of place
        ref, = run_gemm(data, 370, 768, 192)
    same_bits((out,), (ref,), "in place against out of place")


def test_dropout_instantiation_bits(data):
    ab(lambda: run_gemm(data, 193, 768, 192, epi=EPI_BIAS | EPI_RESIDUAL | EPI_DROPOUT), "gemm EPI_DROPOUT", 193)


@pytest.mark.parametrize("K", [128, 768])
def test_new_form_against_fp64(data, K):
    """The bound of tests/test_kernels_gpu.py for the same entry points (fp32 output of bf16 operands against the fp64 product: 2e-5)."""
    M, N = 193, 768
    A, W, b = operands(data, M, N, K)
    ref = A.double() @ W.double().t() + b.double() + data["R"][:M, :N].double()
    with Tune(k0=60, k14=1):
        out, = run_gemm(data, M, N, K)
        out2, outb, part = run_rowstat(data, M, N, K)
    e1, e2 = rel_err(out[:M], ref), rel_err(out2[:M], ref)
    print(f"K={K}: rel err gemm {e1:.3e} rowstat {e2:.3e}")
    assert e1 < 2e-5 and e2 < 2e-5
    assert torch.equal(outb[:M], out2[:M].to(torch.bfloat16))


def test_multi_tile_launch_keeps_the_register_form(data):
    """128 workgroups (key 1 = 128 reserved CUs) for 40 x 4 = 160 tiles: some workgroups walk two tiles, which the new form cannot do."""
    M, N, K = 7680, 768, 128
    A, W, b = rnd(M, K, seed=11).to(torch.bfloat16), data["W"][:N, :K].contiguous(), data["b"][:N].contiguous()
    R = rnd(M, N, seed=12, scale=2.0)

    def run():
        out, outb = sentinel(M, N), sentinel(M, N, torch.bfloat16)
        part = torch.full((M + GUARD, 4 * (N // 192), 2), 7.0, device=DEV)
        check(lib.rmcl_linear_rowstat(P(A), P(W), P(b), P(R), P(out), P(outb), P(part), M, N, K, stream()), "linear_rowstat")
        return out, outb, part
    out, _, _ = ab(run, "160 tiles on 128 workgroups", M, k1=128)
    assert rel_err(out[:M], A.double() @ W.double().t() + b.double() + R.double()) < 2e-5


def test_encoder_infer_pass_cls_rows_bits():
    """2 layers, B = 4, bf16, INFER with the LayerNorm fold on (key 0 = 60 puts every GEMM of the pass on the 192-row tile kernels):
    4 x 4 = 16 tiles per producer launch, one per workgroup."""
    import rmcl_pkg  # noqa: F401
    from oracle import rmcl_oracle as O
    from rmcl_amd.vilt.config import task_moco
    from rmcl_amd.vilt.modules import ViLTransformerSS
    Bn = 4
    ocfg = O.default_config(num_layers=2, num_negative=1024, per_gpu_batchsize=Bn)
    cfg = task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=Bn, drop_rate=0.0, image_view=True, num_gpus=1, num_nodes=1)
    m = ViLTransformerSS(cfg, device=DEV, compute_dtype="bf16")
    m.load_state_dict({n: t.to(DEV) for n, t in O.init_params(ocfg, 3).items()}, strict=False)
    batch = O.synthetic_batch(ocfg, Bn, 4)
    eng = m.engine
    assert eng.fold, "the LayerNorm fold is off"
    eng.dropout_on = False
    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0])
    op = eng.make_operand(pb, out=pb.patchesT_full)
    assert lib.rmcl_gemm_route(Bn * 185, 768, 768, EPI_BIAS | EPI_RESIDUAL | 4096, L.F32, 1, 1) != 1      # (default routing: too few tiles)
    xn = {}
    for key14 in (1, 0, 1):
        with Tune(k0=60, k14=key14):
            assert lib.rmcl_gemm_route(Bn * 185, 768, 768, EPI_BIAS | EPI_RESIDUAL | 4096, L.F32, 1, 1) == 1
            eng.encoder_forward(pb, key=False, mode=L.MODE_INFER, patchesT=op)
            torch.cuda.synchronize()
        cls = pb.xn.view(Bn, -1, 768)[:, 0].clone()
        assert bool(torch.isfinite(cls).all())
        if key14 in xn:
            same_bits((xn[key14],), (cls,), "encoder repeat")
        xn[key14] = cls
    same_bits((xn[1],), (xn[0],), "encoder cls rows")
