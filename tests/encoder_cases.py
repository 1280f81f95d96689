"""Cases, references, metric and bounds shared by tests/test_encoder_fp64_gpu.py (the kernels, on the GPU) and tests/test_encoder_ref_cpu.py
(the reference and the rounding model, on the CPU).  Nothing here touches a device: the library is loaded for rmcl_param_layout only."""
import ctypes as C
import functools

import torch

import rmcl_pkg  # noqa: F401
from oracle import rmcl_oracle as O
from rmcl_amd import _lib as L
from rmcl_amd._lib import lib
from tests import encoder_ref as R

F32_FACTOR, F32_FLOOR, BF16_FACTOR = 8.0, 2.0 ** -23, 3.0
MASK_TOKEN = "moco_head.projector.0.bias"          # a [D] slot of the arena no encoder pass touches: the mask token of the _mpp forms
MODES = {"infer": L.MODE_INFER, "data": L.MODE_DATA, "full": L.MODE_FULL}

SHAPES = {
    "A": dict(D=64, H=1, mlp=64, B=3, L=5, P=9),
    "B": dict(D=320, H=5, mlp=192, B=2, L=4, P=6),
    "C": dict(D=1024, H=16, mlp=64, layers=1, B=1, L=3, P=4),
    "D": dict(D=128, H=2, mlp=256, B=4, L=5, P=16, Pp=16, ragged=True),
    "E2": dict(D=128, H=2, mlp=256, B=3, L=5, P=9, n_types=3, img_type=2),
    "Ep": dict(D=128, H=2, mlp=256, B=4, L=5, P=9, n_types=3, img_type=-1),
    "I": dict(D=128, H=2, mlp=256, B=4, L=5, P=16, Pp=16, ragged=True, rank=(2, 0, 3, 7, 1)),
    "J": dict(D=128, H=2, mlp=256, B=3, L=5, P=9, bf16=True),
    "K": dict(D=192, H=3, mlp=768, B=5, L=24, P=48, bf16=True),
    "K2": dict(D=384, H=6, mlp=768, B=5, L=24, P=48, bf16=True),
    "L4": dict(D=768, H=12, mlp=768, B=4, L=15, P=48, bf16=True),
    "L3": dict(D=768, H=12, mlp=768, B=3, L=15, P=48, bf16=True),
}
GRIDS = ((4, 4), (1, 4), (4, 1), (2, 3))             # valid patch rows x columns per sample of the ragged cases; G0 = 4
REPLACED_A = ((0,) * 9, (0, 1, 0, 0, 1, 1, 0, 0, 1), (1,) * 9)


class EncCase:
    """Inputs of one case on the CPU (fp32 masters; bf16-valued patches on a bf16 arm)."""

    def __init__(self, name):
        kw = dict(SHAPES[name])
        self.name, self.bf16 = name, kw.pop("bf16", False)
        self.is_ragged, self.rank = kw.pop("ragged", False), kw.pop("rank", None)
        kw.setdefault("layers", 2)
        self.dims = d = R.dims_of(vocab=64, patch_k=192, dtype=L.BF16 if self.bf16 else L.F32, exact=0 if self.bf16 else 1, **kw)
        self.cd = L.Dims(**vars(d))
        self.lay = L.Layout()
        lib.rmcl_param_layout(C.byref(self.cd), C.byref(self.lay))
        self.total = int(self.lay.total)
        self.specs = R.arena_specs(d, self.lay)
        self.offs = {n: (o, s) for n, o, s in self.specs}
        seed = 1000 + sorted(SHAPES).index(name)
        self.arena = R.init_arena(self.specs, self.total, seed)
        g = torch.Generator().manual_seed(seed + 500)
        B, Lt, Pn, D = d.B, d.L, d.P, d.D
        self.N = Lt + 1 + Pn
        Bt = len(self.rank) if self.rank else B              # sequences of the pass (the rank pass pairs Bt captions with B cached images)
        self.Bt = Bt
        if name == "A":
            ids = torch.tensor([[7, 7, 12, 0, 3], [12, 0, 0, 0, 0], [7, 20, 20, 5, 0]])
            tm = torch.tensor([[1, 1, 1, 1, 1], [1, 0, 0, 0, 0], [1, 1, 1, 1, 0]])
        else:
            ids = torch.randint(1, 64, (Bt, Lt), generator=g)
            tm = torch.ones(Bt, Lt, dtype=torch.int64)
            ids[0, 1] = ids[0, 0]
            ids[Bt - 1, Lt - 1] = ids[0, 0]
            if Bt > 1:
                tm[1, max(1, Lt // 2):] = 0
                ids[1, max(1, Lt // 2):] = 0
        self.text_ids, self.text_mask = ids.long(), tm.long()
        self.ragged = None
        if self.is_ragged:
            img = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
            for b, (h, w) in enumerate(GRIDS):
                img[b, :, 8 * h:, :] = 0
                img[b, :, :, 8 * w:] = 0
            self.img = img
            m, xh, xw = O.ragged_geometry(img, 8)
            sel, n = O.ragged_select(m, -1)
            assert n == Pn
            sel[0] = sel[0][torch.randperm(Pn, generator=g)]                 # an explicit selection, shared with the reference
            counts = m.flatten(1).sum(1)
            pat = O.patchify(img, 8)
            rows = torch.stack([pat[b, sel[b]] for b in range(B)])
            rows = rows * (torch.arange(Pn)[None, :] < counts[:, None]).float()[:, :, None]
            self.ragged = dict(sel=sel.int(), counts=counts.int(), hw=torch.stack([xh, xw], 1).int(), gw=4, G0=4)
            patches = rows.reshape(B * Pn, 192)
        else:
            patches = torch.rand(B * Pn, 192, generator=g) * 2 - 1
            if name == "A":
                patches[2 * Pn + Pn - 1] = 0                                  # a pad patch: image mask 0
        self.patches = R.bf(patches) if self.bf16 else patches
        self.dxn = torch.randn(Bt, self.N, D, generator=g)
        self.dxn_cls = torch.zeros_like(self.dxn)
        self.dxn_cls[:, 0] = self.dxn[:, 0]
        self.gen = g

    def ref_kw(self, **over):
        kw = dict(ragged=self.ragged, img_of=self.rank)
        kw.update(over)
        return kw


@functools.lru_cache(maxsize=None)
def get_case(name):
    return EncCase(name)


def _freeze(v):
    return tuple(sorted((k, _freeze(x)) for k, x in v.items())) if isinstance(v, dict) else v


@functools.lru_cache(maxsize=None)
def _reference(name, kind, dxn_kind, extra):
    """kind: f64 / f32 / model.  dxn_kind: None (forward only), "full", "cls".  extra: frozen keyword arguments of encoder_ref."""
    c = get_case(name)
    kw = c.ref_kw(**dict(extra))
    if "replaced" in kw:
        kw["replaced"] = torch.tensor(kw["replaced"])
    dxn = {None: None, "full": c.dxn, "cls": c.dxn_cls}[dxn_kind]
    dt = {"f64": torch.float64, "f32": torch.float32, "model": torch.float32}[kind]
    return R.grads(c.arena, c.specs, c.dims, c.text_ids, c.text_mask, c.patches, dxn, dt, model=kind == "model", **kw)


def reference(name, kind, dxn_kind="full", **extra):
    return _reference(name, kind, dxn_kind, _freeze(extra))


def grad_start(c, ref64):
    """The non-zero start of the gradient arena: per tensor, noise of the rms of its reference gradient (1e-3 where that is zero)."""
    g = torch.Generator().manual_seed(77)
    G0 = torch.randn(c.total, generator=g) * 1e-3
    for name, off, shape in c.specs:
        n = R.numel(shape)
        rms = float(ref64["G"][off:off + n].square().mean().sqrt())
        if rms > 0:
            G0[off:off + n] *= rms / 1e-3
    return G0


# ------------------------------------------------------------------------------------------ metric
def row_err(got, ref):
    got, ref = got.double(), ref.double()
    rn = ref.norm(dim=1)
    rms = float(rn.square().mean().sqrt()) or 1e-30
    return float(((got - ref).norm(dim=1) / rn.clamp_min(0.05 * rms)).max())


def blocks(c, res, G0=None, tail=False, added=False):
    """{block: [rows, cols] tensor} of a result dict (xn, dpatches, dtext, G as present).  The G blocks hold the GRADIENT: res["G"] itself
    (G0 None), or what a pass that starts from G0 adds - added = False: res["G"] is a gradient, accumulated onto G0 in its own precision
    and G0 taken off again in float64 (the yardsticks: the rounding of the accumulation is part of them); added = True: res["G"] is the
    arena after the pass (the kernel)."""
    d = c.dims
    out = {}
    xn = res["xn"].reshape(c.Bt, c.N, d.D)
    if tail:
        out["xn_cls"] = xn[:, 0]
    else:
        out["xn_text"], out["xn_image"] = xn[:, :d.L].reshape(-1, d.D), xn[:, d.L:].reshape(-1, d.D)
    for k in ("dpatches", "dtext"):
        if res.get(k) is not None:
            out[k] = res[k].reshape(-1, res[k].shape[-1])
    if res.get("G") is not None:
        G = res["G"]
        if G0 is not None:
            G = (G if added else G0.to(G.dtype) + G).double() - G0.double()
        for name, off, shape in c.specs:
            s = [v for v in shape]
            while len(s) > 1 and s[0] == 1:
                s.pop(0)
            out["G:" + name] = G[off:off + R.numel(shape)].view(s[0] if len(s) > 1 else 1, -1)
    return out


def allowance(bf16, yard):
    """The bound of a block from its yardstick figure (docstring): fp32 arms 8 * max(e32, 2^-23); bf16 arms 3 * model, not below the fp32
    arms' floor where the model moves at all, and exactly 0 where it does not (a tensor the pass must leave alone)."""
    if not bf16:
        return F32_FACTOR * max(yard, F32_FLOOR)
    return max(BF16_FACTOR * yard, F32_FACTOR * F32_FLOOR) if yard > 0 else 0.0


def pick(res, keys):
    return {k: res[k] for k in keys}


def keys_of(mode):
    return ("xn",) if mode == L.MODE_INFER else ("xn", "dpatches", "dtext") + (("G",) if mode == L.MODE_FULL else ())


# label -> (case, mode, keyword arguments of the reference) of the bf16 arms; tests/test_encoder_ref_cpu.py caps the model on each
BF16_VARIANTS = {"J:data": ("J", "data", {}), "J:full": ("J", "full", {}), "K:infer:fold_given": ("K", "infer", {}),
                 "K:data:fold_given": ("K", "data", {}), "K:infer:fold60": ("K", "infer", {"fold": True}), "K:data:fold60": ("K", "data", {"fold": True}),
                 "K2:infer:fold60": ("K2", "infer", {"fold": True}), "K2:data:fold60": ("K2", "data", {"fold": True}), "K:full": ("K", "full", {}), "L4:full": ("L4", "full", {}),
                 "L3:full": ("L3", "full", {}),
                 # the cls-only tail: dxn on the cls rows, xn compared on them (tail = True: the model's switch, tests/encoder_ref.py)
                 "J:cls_tail:data": ("J", "data", {"tail": True}), "L4:cls_tail:full": ("L4", "full", {"tail": True})}


def model_figures(label):
    """{block: worst-row deviation of the rounding model from float64} of a bf16 variant, on the CPU."""
    name, mode, extra = BF16_VARIANTS[label]
    tail = bool(extra.get("tail"))
    c, dk = get_case(name), (None if mode == "infer" else "cls" if tail else "full")
    ref = reference(name, "f64", dk, **extra)
    G0 = grad_start(c, ref) if mode == "full" else None
    keys = keys_of(MODES[mode])
    rb, mb = blocks(c, pick(ref, keys), None, tail), blocks(c, pick(reference(name, "model", dk, **extra), keys), G0, tail)
    return {b: row_err(mb[b], rb[b]) for b in rb}


# Worst-row deviation of the rounding model from float64, per variant and per BLOCK (every layer's tensors on their own), measured on the CPU
# when tests/test_encoder_ref_cpu.py was written; MODEL_CAPS, twice each figure, is what that test holds the model to.
MODEL_MEASURED = {
    "J:data": {
        "dpatches": 3.75e-03, "dtext": 7.59e-04, "xn_image": 2.80e-03, "xn_text": 2.35e-04},
    "J:full": {
        "G:itm_score.fc.bias": 0.00e+00, "G:itm_score.fc.weight": 0.00e+00, "G:moco_head.projector.0.bias": 0.00e+00,
        "G:moco_head.projector.0.weight": 0.00e+00, "G:moco_head.projector.1.bias": 0.00e+00, "G:moco_head.projector.1.weight": 0.00e+00,
        "G:moco_head.projector.3.weight": 0.00e+00, "G:pooler.dense.bias": 0.00e+00, "G:pooler.dense.weight": 0.00e+00,
        "G:text_embeddings.LayerNorm.bias": 9.40e-04, "G:text_embeddings.LayerNorm.weight": 7.62e-04,
        "G:text_embeddings.position_embeddings.weight": 7.40e-04, "G:text_embeddings.token_type_embeddings.weight": 9.50e-04,
        "G:text_embeddings.word_embeddings.weight": 7.60e-04, "G:token_type_embeddings.weight": 3.35e-03,
        "G:transformer.blocks.0.attn.proj.bias": 3.56e-03, "G:transformer.blocks.0.attn.proj.weight": 2.58e-02,
        "G:transformer.blocks.0.attn.qkv.bias": 4.07e-03, "G:transformer.blocks.0.attn.qkv.weight": 2.55e-02,
        "G:transformer.blocks.0.mlp.fc1.bias": 3.98e-03, "G:transformer.blocks.0.mlp.fc1.weight": 9.86e-03,
        "G:transformer.blocks.0.mlp.fc2.bias": 2.46e-03, "G:transformer.blocks.0.mlp.fc2.weight": 6.60e-03,
        "G:transformer.blocks.0.norm1.bias": 5.03e-03, "G:transformer.blocks.0.norm1.weight": 5.46e-03,
        "G:transformer.blocks.0.norm2.bias": 4.28e-03, "G:transformer.blocks.0.norm2.weight": 4.81e-03,
        "G:transformer.blocks.1.attn.proj.bias": 2.37e-03, "G:transformer.blocks.1.attn.proj.weight": 1.97e-02,
        "G:transformer.blocks.1.attn.qkv.bias": 3.73e-03, "G:transformer.blocks.1.attn.qkv.weight": 7.19e-02,
        "G:transformer.blocks.1.mlp.fc1.bias": 3.15e-03, "G:transformer.blocks.1.mlp.fc1.weight": 7.87e-03,
        "G:transformer.blocks.1.mlp.fc2.bias": 1.70e-03, "G:transformer.blocks.1.mlp.fc2.weight": 6.59e-03,
        "G:transformer.blocks.1.norm1.bias": 4.82e-03, "G:transformer.blocks.1.norm1.weight": 5.37e-03,
        "G:transformer.blocks.1.norm2.bias": 4.30e-03, "G:transformer.blocks.1.norm2.weight": 4.66e-03, "G:transformer.cls_token": 3.75e-03,
        "G:transformer.norm.bias": 8.70e-08, "G:transformer.norm.weight": 1.73e-03, "G:transformer.patch_embed.proj.bias": 2.68e-03,
        "G:transformer.patch_embed.proj.weight": 3.00e-03, "G:transformer.pos_embed": 3.75e-03, "dpatches": 3.75e-03, "dtext": 7.59e-04,
        "xn_image": 2.80e-03, "xn_text": 2.35e-04},
    "K:infer:fold_given": {
        "xn_image": 3.90e-03, "xn_text": 4.66e-04},
    "K:data:fold_given": {
        "dpatches": 4.66e-03, "dtext": 6.65e-04, "xn_image": 3.90e-03, "xn_text": 4.66e-04},
    "K:infer:fold60": {
        "xn_image": 3.97e-03, "xn_text": 4.50e-04},
    "K:data:fold60": {
        "dpatches": 4.82e-03, "dtext": 6.63e-04, "xn_image": 3.97e-03, "xn_text": 4.50e-04},
    "K2:infer:fold60": {
        "xn_image": 4.70e-03, "xn_text": 7.03e-04},
    "K2:data:fold60": {
        "dpatches": 5.58e-03, "dtext": 1.24e-03, "xn_image": 4.70e-03, "xn_text": 7.03e-04},
    "K:full": {
        "G:itm_score.fc.bias": 0.00e+00, "G:itm_score.fc.weight": 0.00e+00, "G:moco_head.projector.0.bias": 0.00e+00,
        "G:moco_head.projector.0.weight": 0.00e+00, "G:moco_head.projector.1.bias": 0.00e+00, "G:moco_head.projector.1.weight": 0.00e+00,
        "G:moco_head.projector.3.weight": 0.00e+00, "G:pooler.dense.bias": 0.00e+00, "G:pooler.dense.weight": 0.00e+00,
        "G:text_embeddings.LayerNorm.bias": 1.15e-03, "G:text_embeddings.LayerNorm.weight": 6.32e-04,
        "G:text_embeddings.position_embeddings.weight": 6.42e-04, "G:text_embeddings.token_type_embeddings.weight": 1.14e-03,
        "G:text_embeddings.word_embeddings.weight": 6.80e-04, "G:token_type_embeddings.weight": 3.04e-03,
        "G:transformer.blocks.0.attn.proj.bias": 3.29e-03, "G:transformer.blocks.0.attn.proj.weight": 2.13e-02,
        "G:transformer.blocks.0.attn.qkv.bias": 4.56e-03, "G:transformer.blocks.0.attn.qkv.weight": 2.73e-02,
        "G:transformer.blocks.0.mlp.fc1.bias": 3.65e-03, "G:transformer.blocks.0.mlp.fc1.weight": 6.38e-03,
        "G:transformer.blocks.0.mlp.fc2.bias": 2.37e-03, "G:transformer.blocks.0.mlp.fc2.weight": 5.76e-03,
        "G:transformer.blocks.0.norm1.bias": 4.33e-03, "G:transformer.blocks.0.norm1.weight": 4.69e-03,
        "G:transformer.blocks.0.norm2.bias": 4.11e-03, "G:transformer.blocks.0.norm2.weight": 4.49e-03,
        "G:transformer.blocks.1.attn.proj.bias": 2.35e-03, "G:transformer.blocks.1.attn.proj.weight": 1.64e-02,
        "G:transformer.blocks.1.attn.qkv.bias": 2.85e-03, "G:transformer.blocks.1.attn.qkv.weight": 2.13e-02,
        "G:transformer.blocks.1.mlp.fc1.bias": 3.16e-03, "G:transformer.blocks.1.mlp.fc1.weight": 6.05e-03,
        "G:transformer.blocks.1.mlp.fc2.bias": 1.60e-03, "G:transformer.blocks.1.mlp.fc2.weight": 5.08e-03,
        "G:transformer.blocks.1.norm1.bias": 3.21e-03, "G:transformer.blocks.1.norm1.weight": 3.76e-03,
        "G:transformer.blocks.1.norm2.bias": 3.72e-03, "G:transformer.blocks.1.norm2.weight": 4.82e-03, "G:transformer.cls_token": 4.39e-03,
        "G:transformer.norm.bias": 1.19e-07, "G:transformer.norm.weight": 2.11e-03, "G:transformer.patch_embed.proj.bias": 3.16e-03,
        "G:transformer.patch_embed.proj.weight": 4.03e-03, "G:transformer.pos_embed": 4.39e-03, "dpatches": 4.66e-03, "dtext": 6.65e-04,
        "xn_image": 3.90e-03, "xn_text": 4.66e-04},
    "L4:full": {
        "G:itm_score.fc.bias": 0.00e+00, "G:itm_score.fc.weight": 0.00e+00, "G:moco_head.projector.0.bias": 0.00e+00,
        "G:moco_head.projector.0.weight": 0.00e+00, "G:moco_head.projector.1.bias": 0.00e+00, "G:moco_head.projector.1.weight": 0.00e+00,
        "G:moco_head.projector.3.weight": 0.00e+00, "G:pooler.dense.bias": 0.00e+00, "G:pooler.dense.weight": 0.00e+00,
        "G:text_embeddings.LayerNorm.bias": 3.76e-03, "G:text_embeddings.LayerNorm.weight": 2.64e-03,
        "G:text_embeddings.position_embeddings.weight": 1.97e-03, "G:text_embeddings.token_type_embeddings.weight": 3.73e-03,
        "G:text_embeddings.word_embeddings.weight": 2.52e-03, "G:token_type_embeddings.weight": 5.24e-03,
        "G:transformer.blocks.0.attn.proj.bias": 4.68e-03, "G:transformer.blocks.0.attn.proj.weight": 3.47e-02,
        "G:transformer.blocks.0.attn.qkv.bias": 4.98e-03, "G:transformer.blocks.0.attn.qkv.weight": 4.08e-02,
        "G:transformer.blocks.0.mlp.fc1.bias": 4.65e-03, "G:transformer.blocks.0.mlp.fc1.weight": 1.15e-02,
        "G:transformer.blocks.0.mlp.fc2.bias": 3.61e-03, "G:transformer.blocks.0.mlp.fc2.weight": 8.82e-03,
        "G:transformer.blocks.0.norm1.bias": 5.48e-03, "G:transformer.blocks.0.norm1.weight": 5.98e-03,
        "G:transformer.blocks.0.norm2.bias": 5.41e-03, "G:transformer.blocks.0.norm2.weight": 5.46e-03,
        "G:transformer.blocks.1.attn.proj.bias": 2.99e-03, "G:transformer.blocks.1.attn.proj.weight": 3.69e-02,
        "G:transformer.blocks.1.attn.qkv.bias": 3.91e-03, "G:transformer.blocks.1.attn.qkv.weight": 3.35e-02,
        "G:transformer.blocks.1.mlp.fc1.bias": 3.71e-03, "G:transformer.blocks.1.mlp.fc1.weight": 1.05e-02,
        "G:transformer.blocks.1.mlp.fc2.bias": 1.80e-03, "G:transformer.blocks.1.mlp.fc2.weight": 6.81e-03,
        "G:transformer.blocks.1.norm1.bias": 4.23e-03, "G:transformer.blocks.1.norm1.weight": 4.91e-03,
        "G:transformer.blocks.1.norm2.bias": 4.32e-03, "G:transformer.blocks.1.norm2.weight": 5.34e-03, "G:transformer.cls_token": 5.86e-03,
        "G:transformer.norm.bias": 1.15e-07, "G:transformer.norm.weight": 3.31e-03, "G:transformer.patch_embed.proj.bias": 5.12e-03,
        "G:transformer.patch_embed.proj.weight": 6.28e-03, "G:transformer.pos_embed": 5.86e-03, "dpatches": 6.25e-03, "dtext": 2.11e-03,
        "xn_image": 4.86e-03, "xn_text": 1.09e-03},
    "L3:full": {
        "G:itm_score.fc.bias": 0.00e+00, "G:itm_score.fc.weight": 0.00e+00, "G:moco_head.projector.0.bias": 0.00e+00,
        "G:moco_head.projector.0.weight": 0.00e+00, "G:moco_head.projector.1.bias": 0.00e+00, "G:moco_head.projector.1.weight": 0.00e+00,
        "G:moco_head.projector.3.weight": 0.00e+00, "G:pooler.dense.bias": 0.00e+00, "G:pooler.dense.weight": 0.00e+00,
        "G:text_embeddings.LayerNorm.bias": 3.44e-03, "G:text_embeddings.LayerNorm.weight": 2.60e-03,
        "G:text_embeddings.position_embeddings.weight": 2.06e-03, "G:text_embeddings.token_type_embeddings.weight": 3.45e-03,
        "G:text_embeddings.word_embeddings.weight": 2.32e-03, "G:token_type_embeddings.weight": 4.92e-03,
        "G:transformer.blocks.0.attn.proj.bias": 4.28e-03, "G:transformer.blocks.0.attn.proj.weight": 4.89e-02,
        "G:transformer.blocks.0.attn.qkv.bias": 4.85e-03, "G:transformer.blocks.0.attn.qkv.weight": 6.19e-02,
        "G:transformer.blocks.0.mlp.fc1.bias": 4.44e-03, "G:transformer.blocks.0.mlp.fc1.weight": 1.06e-02,
        "G:transformer.blocks.0.mlp.fc2.bias": 3.61e-03, "G:transformer.blocks.0.mlp.fc2.weight": 9.19e-03,
        "G:transformer.blocks.0.norm1.bias": 5.18e-03, "G:transformer.blocks.0.norm1.weight": 5.61e-03,
        "G:transformer.blocks.0.norm2.bias": 4.68e-03, "G:transformer.blocks.0.norm2.weight": 5.50e-03,
        "G:transformer.blocks.1.attn.proj.bias": 3.00e-03, "G:transformer.blocks.1.attn.proj.weight": 4.18e-02,
        "G:transformer.blocks.1.attn.qkv.bias": 3.77e-03, "G:transformer.blocks.1.attn.qkv.weight": 5.24e-02,
        "G:transformer.blocks.1.mlp.fc1.bias": 3.67e-03, "G:transformer.blocks.1.mlp.fc1.weight": 1.32e-02,
        "G:transformer.blocks.1.mlp.fc2.bias": 1.60e-03, "G:transformer.blocks.1.mlp.fc2.weight": 7.56e-03,
        "G:transformer.blocks.1.norm1.bias": 4.10e-03, "G:transformer.blocks.1.norm1.weight": 4.97e-03,
        "G:transformer.blocks.1.norm2.bias": 4.38e-03, "G:transformer.blocks.1.norm2.weight": 5.89e-03, "G:transformer.cls_token": 5.71e-03,
        "G:transformer.norm.bias": 1.00e-07, "G:transformer.norm.weight": 3.38e-03, "G:transformer.patch_embed.proj.bias": 4.93e-03,
        "G:transformer.patch_embed.proj.weight": 6.63e-03, "G:transformer.pos_embed": 5.71e-03, "dpatches": 6.67e-03, "dtext": 2.27e-03,
        "xn_image": 4.95e-03, "xn_text": 1.07e-03},
    "J:cls_tail:data": {
        "dpatches": 5.69e-03, "dtext": 9.41e-04, "xn_cls": 1.67e-04},
    "L4:cls_tail:full": {
        "G:itm_score.fc.bias": 0.00e+00, "G:itm_score.fc.weight": 0.00e+00, "G:moco_head.projector.0.bias": 0.00e+00,
        "G:moco_head.projector.0.weight": 0.00e+00, "G:moco_head.projector.1.bias": 0.00e+00, "G:moco_head.projector.1.weight": 0.00e+00,
        "G:moco_head.projector.3.weight": 0.00e+00, "G:pooler.dense.bias": 0.00e+00, "G:pooler.dense.weight": 0.00e+00,
        "G:text_embeddings.LayerNorm.bias": 8.82e-04, "G:text_embeddings.LayerNorm.weight": 8.23e-04,
        "G:text_embeddings.position_embeddings.weight": 3.41e-03, "G:text_embeddings.token_type_embeddings.weight": 8.78e-04,
        "G:text_embeddings.word_embeddings.weight": 4.82e-03, "G:token_type_embeddings.weight": 3.63e-03,
        "G:transformer.blocks.0.attn.proj.bias": 2.65e-03, "G:transformer.blocks.0.attn.proj.weight": 3.03e-02,
        "G:transformer.blocks.0.attn.qkv.bias": 3.14e-03, "G:transformer.blocks.0.attn.qkv.weight": 4.33e-02,
        "G:transformer.blocks.0.mlp.fc1.bias": 3.29e-03, "G:transformer.blocks.0.mlp.fc1.weight": 3.17e-02,
        "G:transformer.blocks.0.mlp.fc2.bias": 2.07e-03, "G:transformer.blocks.0.mlp.fc2.weight": 1.14e-02,
        "G:transformer.blocks.0.norm1.bias": 3.62e-03, "G:transformer.blocks.0.norm1.weight": 3.99e-03, "G:transformer.blocks.0.norm2.bias": 4.07e-03,
        "G:transformer.blocks.0.norm2.weight": 4.05e-03, "G:transformer.blocks.1.attn.proj.bias": 8.30e-05,
        "G:transformer.blocks.1.attn.proj.weight": 5.88e-03, "G:transformer.blocks.1.attn.qkv.bias": 1.72e-03,
        "G:transformer.blocks.1.attn.qkv.weight": 6.30e-02, "G:transformer.blocks.1.mlp.fc1.bias": 4.08e-04,
        "G:transformer.blocks.1.mlp.fc1.weight": 1.00e-02, "G:transformer.blocks.1.mlp.fc2.bias": 3.59e-05,
        "G:transformer.blocks.1.mlp.fc2.weight": 1.33e-03, "G:transformer.blocks.1.norm1.bias": 2.42e-03,
        "G:transformer.blocks.1.norm1.weight": 3.75e-03, "G:transformer.blocks.1.norm2.bias": 3.92e-04,
        "G:transformer.blocks.1.norm2.weight": 8.22e-04, "G:transformer.cls_token": 4.81e-03, "G:transformer.norm.bias": 6.01e-08,
        "G:transformer.norm.weight": 7.75e-04, "G:transformer.patch_embed.proj.bias": 3.61e-03, "G:transformer.patch_embed.proj.weight": 1.37e-02,
        "G:transformer.pos_embed": 5.04e-03, "dpatches": 6.56e-03, "dtext": 3.83e-03, "xn_cls": 7.88e-04},
}
MODEL_CAPS = {label: {b: 2.0 * v for b, v in fig.items()} for label, fig in MODEL_MEASURED.items()}
