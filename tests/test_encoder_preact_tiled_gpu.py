"""-m gpu: an encoder pass with the MLP pre-activation stash in tile order (rmcl_tune_set key 15 = 1, the default) against the same pass
with the row-major stash (key 15 = 0), at the smallest encoder whose MLP GEMMs run on the 192x384 kernel: D = 192, mlp = 768, 3 heads,
2 layers, B x N = 5 x 73 = 365 rows (two uneven row tiles, 19 rows short of whole blocks - few enough for the tiled buffer's
padding to fit in front of a layer's slot, in the free tail of its attention-statistics slot: at 3 x 65 rows it does not, and the encoder
keeps the row-major stash).  Key 0 = 70 routes fc1 and fc2-dX there at this size.  The two forms
compute the same values in the same order: whatever has no atomics on its path - the data gradient, the cls rows of xn - is compared bit
for bit; the parameter gradients of a FULL pass (split-K sums through fp32 atomics) against the spread of two runs of one setting."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, stream  # noqa: E402

EPI_BIAS, EPI_GELU, EPI_SAVE_PREACT, EPI_DGELU, EPI_TILED = 1, 2, 4, 16, 16384
B, LT, PN, D, MLP, LAYERS = 5, 24, 48, 192, 768, 2
N = LT + 1 + PN


class Case:
    def __init__(self):
        self.d = d = L.Dims(B=B, L=LT, P=PN, D=D, H=D // 64, layers=LAYERS, mlp=MLP, patch_k=192, proj=128, vocab=128, dtype=L.BF16, exact=0,
                            Pp=PN, n_types=0, img_type=0)
        self.lay = lay = L.Layout()
        lib.rmcl_param_layout(C.byref(d), C.byref(lay))
        g = torch.Generator().manual_seed(5)
        p = torch.randn(int(lay.total), generator=g) * 0.05
        for off in [lay.eln_w, lay.norm_w] + [lay.layer0 + l * lay.layer_stride + o for l in range(LAYERS) for o in (lay.ln1_w, lay.ln2_w)]:
            p[off:off + D] += 1.0
        self.p32 = p.to(DEV)
        self.plp = self.p32.bfloat16()
        self.plpT = torch.zeros_like(self.plp)
        check(lib.rmcl_weight_transpose_bf16(C.byref(d), P(self.plp), P(self.plpT), stream()), "weight_transpose")
        self.text_ids = torch.randint(0, 128, (B, LT), generator=g).to(DEV)
        tm = torch.ones(B, LT, dtype=torch.int64)
        tm[1, 9:] = 0
        self.text_mask = tm.to(DEV)
        self.patches = torch.randn(B * PN, d.patch_k, generator=g).to(DEV).bfloat16()
        self.dxn = {True: torch.randn(B, D, generator=g).to(DEV), False: torch.randn(B * N, D, generator=g).to(DEV)}
        self.stash = torch.empty(int(lib.rmcl_stash_bytes(C.byref(d), L.MODE_FULL)), dtype=torch.uint8, device=DEV)
        self.ws = torch.empty(int(lib.rmcl_workspace_bytes(C.byref(d))), dtype=torch.uint8, device=DEV)

    def run(self, mode, tail, drop_p=0.0, tiled=None):
        """tiled = True / False: also check that the forward did / did not take the tiled form - a backward WITHOUT the transposed weight
        shadows is refused for a tiled stash before anything is launched, and only for one."""
        d = self.d
        co = torch.zeros(B, N, dtype=torch.int32, device=DEV)
        xn = torch.zeros(B * N, D, device=DEV)
        seed, p = C.c_uint32(1234), C.c_float(drop_p)
        check(lib.rmcl_encoder_forward(C.byref(d), mode | (L.MODE_CLS_TAIL if tail else 0), P(self.p32), P(self.plp), P(self.text_ids), P(self.text_mask),
                                       P(self.patches), P(co), P(self.stash), P(self.ws), P(xn), seed, p, None, None, stream()), "encoder_forward")
        out = {"dpatches": torch.zeros(B * PN, d.patch_k, dtype=torch.bfloat16, device=DEV), "dtext": torch.zeros(B * LT, D, device=DEV)}
        if mode == L.MODE_FULL:
            out["G"] = torch.zeros(int(self.lay.total), device=DEV)
        check(lib.rmcl_encoder_backward(C.byref(d), mode, P(self.p32), P(self.plp), P(self.text_ids), P(self.patches), P(co), P(self.stash), P(self.ws),
                                        P(self.dxn[tail]), 2 if tail else 0, P(out["dpatches"]), P(out["dtext"]), P(out.get("G")), seed, p, None,
                                        P(self.plpT), stream()), "encoder_backward")
        if tiled:
            rc = lib.rmcl_encoder_backward(C.byref(d), mode, P(self.p32), P(self.plp), P(self.text_ids), P(self.patches), P(co), P(self.stash), P(self.ws),
                                           P(self.dxn[tail]), 2 if tail else 0, P(out["dpatches"]), P(out["dtext"]), P(out.get("G")), seed, p, None,
                                           None, stream())
            assert rc != 0 and b"tiled" in lib.rmcl_last_error(), "the forward did not take the tiled stash"
        torch.cuda.synchronize()
        out["cls"] = xn.view(B, N, D)[:, 0].clone()
        return out


@pytest.fixture(scope="module")
def case():
    return Case()


class Keys:
    """key 0 = 70: the 192x384 kernel wherever it supports the GEMM; key 15: the stash form.  Process-global: restored on the way out."""

    def __init__(self, k15):
        self.k15 = k15

    def __enter__(self):
        check(lib.rmcl_tune_set(0, 70), "tune_set")
        check(lib.rmcl_tune_set(15, self.k15), "tune_set")

    def __exit__(self, *exc):
        check(lib.rmcl_tune_set(0, -1), "tune_set")
        check(lib.rmcl_tune_set(15, 1), "tune_set")


def both(case, mode, tail, drop_p=0.0, repeats=1):
    runs = {}
    for k15 in (0, 1):
        with Keys(k15):
            # the MLP GEMMs of this encoder go to the 192x384 kernel, with the flag when asked to
            flag = EPI_TILED if k15 else 0
            assert lib.rmcl_gemm_route(B * N, MLP, D, EPI_BIAS | EPI_GELU | EPI_SAVE_PREACT | flag, L.BF16, 1, 1) == 2
            assert lib.rmcl_gemm_route(B * N, MLP, D, EPI_DGELU | flag, L.BF16, 1, 1) == 2
            runs[k15] = [case.run(mode, tail, drop_p, tiled=bool(k15)) for _ in range(repeats)]
    return runs


def same(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        assert bool(torch.isfinite(x.float()).all()) and float(x.float().abs().max()) > 0, k
        assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32), y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)), k


def test_data_pass_with_cls_tail_bits(case):
    runs = both(case, L.MODE_DATA, True)
    same(runs[1][0], runs[0][0], ("dpatches", "dtext", "cls"))


def test_data_pass_under_dropout_bits(case):
    """The dropout instantiations: the masks are indexed by the logical element, whatever the layout of the stash."""
    runs = both(case, L.MODE_DATA, False, drop_p=0.1)
    same(runs[1][0], runs[0][0], ("dpatches", "dtext", "cls"))
    clean = both(case, L.MODE_DATA, False)[1][0]
    assert not torch.equal(clean["dpatches"], runs[1][0]["dpatches"])          # (the masks did act)


def test_full_pass_parameter_gradients(case):
    """The weight gradients are sums through fp32 atomics: two runs of ONE setting differ in the last bits, by a few ulp of the largest
    elements, and the distance between two such runs is itself a random draw.  Both settings feed the weight-gradient GEMMs the same bits
    (du, h and the LayerNorm outputs: the data gradient below is compared bit for bit), so a distance between the settings is a draw from
    the same distribution - and a single draw exceeds another single draw half of the time.  Hence three runs per setting: the spread is
    the largest distance between two runs of one setting (six pairs), and the settings count as no further apart than that when some run
    of one is within the spread of some run of the other (nine pairs).  A wrong stash shows in every pair, orders of magnitude above."""
    runs = both(case, L.MODE_FULL, False, repeats=3)
    for r in runs[1]:
        same(r, runs[0][0], ("dpatches", "dtext", "cls"))
    dist = lambda a, b: float((a["G"].double() - b["G"].double()).abs().max())
    spread = max(dist(runs[k][i], runs[k][j]) for k in (0, 1) for i in range(3) for j in range(i))
    cross = [dist(a, b) for a in runs[1] for b in runs[0]]
    print(f"gradient arena: max |d| between settings {min(cross):.3e} .. {max(cross):.3e}, between two runs of one setting up to {spread:.3e} "
          f"(max |G| {float(runs[0][0]['G'].abs().max()):.3e})")
    assert float(runs[0][0]["G"].abs().max()) > 0 and all(bool(torch.isfinite(r["G"]).all()) for r in runs[1])
    assert min(cross) <= spread


def test_backward_reads_the_recorded_layout_not_the_key(case):
    """Key 15 flipped between forward and backward: the backward goes by what the forward recorded with the stash."""
    d = case.d
    with Keys(1):
        want = case.run(L.MODE_DATA, False)
        co = torch.zeros(B, N, dtype=torch.int32, device=DEV)
        xn = torch.zeros(B * N, D, device=DEV)
        check(lib.rmcl_encoder_forward(C.byref(d), L.MODE_DATA, P(case.p32), P(case.plp), P(case.text_ids), P(case.text_mask), P(case.patches), P(co),
                                       P(case.stash), P(case.ws), P(xn), C.c_uint32(0), C.c_float(0.0), None, None, stream()), "encoder_forward")
        check(lib.rmcl_tune_set(15, 0), "tune_set")
        out = {"dpatches": torch.zeros(B * PN, d.patch_k, dtype=torch.bfloat16, device=DEV), "dtext": torch.zeros(B * LT, D, device=DEV)}
        check(lib.rmcl_encoder_backward(C.byref(d), L.MODE_DATA, P(case.p32), P(case.plp), P(case.text_ids), P(case.patches), P(co), P(case.stash),
                                        P(case.ws), P(case.dxn[False]), 0, P(out["dpatches"]), P(out["dtext"]), None, C.c_uint32(0), C.c_float(0.0), None,
                                        P(case.plpT), stream()), "encoder_backward")
        # without the transposed weight shadows a tiled stash cannot be read: refused with a message, nothing launched row-major
        rc = lib.rmcl_encoder_backward(C.byref(d), L.MODE_DATA, P(case.p32), P(case.plp), P(case.text_ids), P(case.patches), P(co), P(case.stash),
                                       P(case.ws), P(case.dxn[False]), 0, P(out["dpatches"]), P(out["dtext"]), None, C.c_uint32(0), C.c_float(0.0), None,
                                       None, stream())
        assert rc != 0 and b"tiled" in lib.rmcl_last_error()
    torch.cuda.synchronize()
    same(out, want, ("dpatches", "dtext"))
