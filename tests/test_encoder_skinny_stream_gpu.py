"""-m gpu: a 2-layer encoder in cls-only-tail mode followed by the pooler / MoCo head, forward and full backward, with the skinny fp32
GEMMs of the tail and the heads in the streaming form (rmcl_tune_set key 6 at its default; the tail's proj then reads the cls rows of the
bf16 attention output in place, no gather launch) against the same pass on the k-split kernel (key 6 = 1).  D = 192, mlp = 768, 3 heads,
N = 24 + 1 + 48 = 73 tokens: the tail's GEMMs have K = 192 (three single-step bursts: a chunk as long as the A ring) and K = 768 (the
12-step burst), both weight layouts.  B = 4 and B = 3: one partial row tile either way, an odd row count once.  Dropout p = 0 and
p = 0.1 (fixed non-zero seed): at 0.1 the tail's GEMMs run their dropout epilogues (EPI_DROPOUT wherever the encoder's with_drop sets it on the tail's proj /
fc1 / fc2 launches, EPI_DROP_BWD in fc2's data gradient, both on compact rows through drop_row_mul) - the one place the two forms' dropout tails are compared at all.

The two forms compute the same values in the same order, and nothing in the forward or in the data gradient sums through atomics:
  * x_final (the cls rows of xn), the whole stash - the compact x_mid, u, h, ln2 and the LayerNorm statistics of the tail live in it -,
    the heads' q and cls_feats, and the data gradients are compared bit for bit;
  * of the parameter gradients, those of the tail's own GEMMs (last layer's proj, fc1, fc2 weights and biases: the short-K kernel, one
    workgroup per element, C += in place) and of the heads bit for bit; the rest of the arena - split-K sums through fp32 atomics - as
    tests/test_encoder_preact_tiled_gpu.py does: three runs per setting, the settings no further apart than two runs of one setting."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV, L, lib, check, P, stream  # noqa: E402

LT, PN, D, MLP, LAYERS, PROJ = 24, 48, 192, 768, 2, 128
N = LT + 1 + PN


class Case:
    def __init__(self, B):
        self.B = B
        self.d = d = L.Dims(B=B, L=LT, P=PN, D=D, H=D // 64, layers=LAYERS, mlp=MLP, patch_k=192, proj=PROJ, vocab=128, dtype=L.BF16, exact=0,
                            Pp=PN, n_types=0, img_type=0)
        self.lay = lay = L.Layout()
        lib.rmcl_param_layout(C.byref(d), C.byref(lay))
        g = torch.Generator().manual_seed(11 + B)
        p = torch.randn(int(lay.total), generator=g) * 0.05
        for off in [lay.eln_w, lay.norm_w, lay.mh1_w] + [lay.layer0 + l * lay.layer_stride + o for l in range(LAYERS) for o in (lay.ln1_w, lay.ln2_w)]:
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
        self.dq = torch.randn(B, PROJ, generator=g).to(DEV)
        self.stash_bytes = int(lib.rmcl_stash_bytes(C.byref(d), L.MODE_FULL))
        self.hstash_bytes = int(lib.rmcl_heads_stash_bytes(C.byref(d)))
        self.ws = torch.empty(int(lib.rmcl_workspace_bytes(C.byref(d))), dtype=torch.uint8, device=DEV)

    def run(self, drop_p=0.0, drop_seed=0):
        d, B = self.d, self.B
        stash = torch.zeros(self.stash_bytes, dtype=torch.uint8, device=DEV)     # zeroed: what a pass leaves unwritten compares equal
        hstash = torch.zeros(self.hstash_bytes + 16, dtype=torch.uint8, device=DEV)
        co = torch.zeros(B, N, dtype=torch.int32, device=DEV)
        xn = torch.zeros(B * N, D, device=DEV)
        seed, p = C.c_uint32(drop_seed), C.c_float(drop_p)
        check(lib.rmcl_encoder_forward(C.byref(d), L.MODE_FULL | L.MODE_CLS_TAIL, P(self.p32), P(self.plp), P(self.text_ids), P(self.text_mask),
                                       P(self.patches), P(co), P(stash), P(self.ws), P(xn), seed, p, None, None, stream()), "encoder_forward")
        cls, q = torch.zeros(B, D, device=DEV), torch.zeros(B, PROJ, device=DEV)
        check(lib.rmcl_heads_forward(C.byref(d), P(self.p32), P(self.p32), P(xn), P(hstash), P(cls), P(q), stream()), "heads_forward")
        out = {"x_final": xn.view(B, N, D)[:, 0].clone(), "stash": stash.clone(), "cls_feats": cls, "q": q}
        G = torch.zeros(int(self.lay.total), device=DEV)
        dcls = torch.zeros(B, D, device=DEV)
        check(lib.rmcl_heads_backward(C.byref(d), P(self.p32), P(self.p32), P(hstash), P(self.dq), None, P(dcls), P(G), P(self.ws), stream()),
              "heads_backward")
        dcls = dcls.clone()                                                      # (the heads' scratch is the start of the encoder workspace)
        out["dpatches"] = torch.zeros(B * PN, d.patch_k, dtype=torch.bfloat16, device=DEV)
        out["dtext"] = torch.zeros(B * LT, D, device=DEV)
        check(lib.rmcl_encoder_backward(C.byref(d), L.MODE_FULL, P(self.p32), P(self.plp), P(self.text_ids), P(self.patches), P(co), P(stash),
                                        P(self.ws), P(dcls), 2, P(out["dpatches"]), P(out["dtext"]), P(G), seed, p, None, P(self.plpT), stream()),
              "encoder_backward")
        torch.cuda.synchronize()
        out["dcls"], out["G"] = dcls, G
        return out

    def owned(self):
        """(offset, length) of the gradient-arena pieces that one workgroup per element writes: the tail's GEMMs and the heads."""
        lay, last = self.lay, self.lay.layer0 + (LAYERS - 1) * self.lay.layer_stride
        pieces = [(last + lay.proj_w, D * D), (last + lay.proj_b, D), (last + lay.fc1_w, MLP * D), (last + lay.fc1_b, MLP), (last + lay.fc2_w, D * MLP),
                  (last + lay.fc2_b, D)]
        pieces += [(lay.pool_w, D * D), (lay.pool_b, D), (lay.mh0_w, D * D), (lay.mh0_b, D), (lay.mh3_w, PROJ * D)]
        return [(int(o), int(n)) for o, n in pieces]


def view_bits(t):
    return t.contiguous().view(torch.uint8)


DROP_SEED = 20241                                  # any non-zero seed: the masks depend on it, the agreement must not


@pytest.mark.parametrize("B", [4, 3])
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_tail_and_heads_on_the_streaming_form_have_the_ksplit_bits(drop_p, B):
    case = Case(B)
    seed = DROP_SEED if drop_p > 0 else 0
    runs = {}
    for form in (1, -1):
        check(lib.rmcl_tune_set(6, form), "tune_set")
        try:
            runs[form] = [case.run(drop_p, seed) for _ in range(3)]
        finally:
            check(lib.rmcl_tune_set(6, -1), "tune_set")
    old, new = runs[1][0], runs[-1][0]
    for k in ("x_final", "q", "cls_feats", "dcls", "dpatches", "dtext"):
        assert bool(torch.isfinite(new[k].float()).all()) and float(new[k].float().abs().max()) > 0, k
    for r in runs[-1]:
        for k in ("x_final", "stash", "q", "cls_feats", "dcls", "dpatches", "dtext"):
            assert torch.equal(view_bits(r[k]), view_bits(old[k])), (B, drop_p, k)
        for off, n in case.owned():
            assert float(old["G"][off:off + n].abs().max()) > 0, off
            assert torch.equal(view_bits(r["G"][off:off + n]), view_bits(old["G"][off:off + n])), (B, drop_p, off)
    dist = lambda a, b: float((a["G"].double() - b["G"].double()).abs().max())
    spread = max(dist(runs[k][i], runs[k][j]) for k in (1, -1) for i in range(3) for j in range(i))
    cross = [dist(a, b) for a in runs[-1] for b in runs[1]]
    print(f"B {B} p {drop_p} gradient arena: max |d| between forms {min(cross):.3e} .. {max(cross):.3e}, between two runs of one form up to {spread:.3e} "
          f"(max |G| {float(old['G'].abs().max()):.3e})")
    assert all(bool(torch.isfinite(r["G"]).all()) for r in runs[-1])
    assert min(cross) <= spread
