"""Plain torch reference of the encoder pass (rmcl_encoder_forward / _backward / _forward_mpp / _forward_rank, rmcl_visual_embed) over the
ARENA: offsets from rmcl_param_layout, names from runtime.param_specs.  TEST INFRASTRUCTURE ONLY, written from csrc/encoder.cpp, csrc/embed_misc.hip
and the comments of include/rmcl.h.

encoder_ref(arena, specs, dims, text_ids, text_mask, patches, ...) -> (xn [B, N, D], co_mask [B, N]) works at the PATCH level
(pe = patches @ patch_w^T + patch_b), so P need not be a square grid.  Its dtype is the arena's: torch.float64 is the reference, torch.float32
the error yardstick of the fp32 arms.  Gradients come from autograd of sum(xn * dxn) (grads()): the arena's .grad IS the gradient arena.

model = True is the rounding model of the bf16 arms (dtype bf16, exact 0), fp32 torch.  q(x) rounds the value to bf16 in the forward and the
incoming gradient to bf16 in the backward (straight-through); qf rounds the value only, qg the gradient only.  They stand wherever
encoder.cpp stores a tensor in the operand type (LayerStash, Work and the backward's du / dqkv / dao / dln / dx copies):
  forward   ln1 = q(LN1(x))            LayerStash.ln1 / Work.ln; its gradient is Work.dln in the operand type
            qkv = q(ln1 Wqkv^T + b)    LayerStash.qkv; the gradient is the attention backward's bf16 dqkv
            attention                  the fused kernels (N <= 256): P and dS in bf16 before the second products, ao = LayerStash.ao and
                                       dqkv in bf16, dao = Work.dao rounded on the way in, delta from the bf16 ao at N <= 192 (the one-kernel
                                       backward) - the rounding_model of tests/test_attention_kernels_gpu.py.  `probs` is stored in the operand
                                       type on the unfused path only (exact = 1 or N > 256): not an arm of the bf16 cases here
            ln2 = q(LN2(x_mid))        LayerStash.ln2 / Work.ln, gradient Work.dln
            u   = qf(pre-activation)   LayerStash.u: the backward's gelu' reads the rounded u; du = Work.du is qg on the pre-activation
            h   = qf(gelu(pre))        LayerStash.h / Work.h (its gradient stays in the fc2-dX accumulators: not rounded)
  backward  the operand copies of dx   every LayerNorm backward writes dx (fp32) and a bf16 copy T: qg on the output of proj and of fc2 -
                                       the dY of their dX, dW and bias-gradient products
            dpe = qg(pe)               Work.dpe (image_assemble_bwd); dpatches = bf16(dpe Wpatch)
  once      patch_w, qkv_w, proj_w, fc1_w, fc2_w (the bf16 shadow arena, straight-through to the fp32 gradient) and the patches
  fp32      the residual stream (x_in, x_mid, x_final, dx), every bias / LayerNorm vector, the embeddings, the text rows, pos / cls / token
            type and their gradients, the mask-token gradient, all weight-gradient accumulation.
fold = True adds the LayerNorm fold of INFER / DATA passes (rmcl_ln_fold: W' = bf16(W gamma) from the fp32 masters, s = rowsum(W'),
c = W beta + b): y = rstd (bf16(x - centre) W'^T - mean(x - centre) s) + c for fc1 of every layer (centre = LN1's row mean) and qkv of the
layers after the first (centre = the previous LN2's row mean); its VALUE replaces the plain form's, the backward is the plain form's
(encoder_backward reads x_in / x_mid and the statistics from the stash and the unfolded bf16 weights).
tail = True is the cls-only tail (RMCL_MODE_CLS_TAIL, backward cls_only = 2): behind the attention of the LAST block the kernel works on the cls
rows alone, in fp32 on the fp32 master weights (exact skinny GEMMs; compact fp32 x_mid, ln2, u, h) - the model drops every rounding there, on
all rows: the block is row-wise behind the attention, only the cls rows of xn are compared and only they carry a gradient.  What stays rounded
is what the kernel still rounds: the attention output (bf16 stash) and its gradient (Work.dao is scatter-cast to the operand type)."""
import math
import types

import torch
import torch.nn.functional as F

from oracle import rmcl_oracle as O

LN_SUFFIXES = ("norm1.weight", "norm2.weight", "norm.weight", "LayerNorm.weight", "projector.1.weight")
MATRICES = ("patch_embed.proj.weight", "attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")


def bf(x):
    return x.bfloat16().to(x.dtype)


class _Q(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf(g) if ctx.bwd else g), None, None


def q(x):
    return _Q.apply(x, True, True)


def qf(x):
    return _Q.apply(x, True, False)


def qg(x):
    return _Q.apply(x, False, True)


class _GeluStash(torch.autograd.Function):
    """gelu(pre) from the fp32 accumulators; the backward multiplies by gelu'(u), u = the bf16 pre-activation of the stash."""
    @staticmethod
    def forward(ctx, pre):
        ctx.save_for_backward(bf(pre))
        return O.gelu_erf(pre)

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return g * (0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))


class _AttnModel(torch.autograd.Function):
    """tests/test_attention_kernels_gpu.py rounding_model on [B, N, 3D] (bf16 values)."""
    @staticmethod
    def forward(ctx, qkv, mask, H):
        B, N, _ = qkv.shape
        t = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        s = (t[0] @ t[1].transpose(-2, -1)) * 0.125
        s = s.masked_fill(~mask.bool()[:, None, None, :], float("-inf"))
        p = s.softmax(-1)
        o = bf(bf(p) @ t[2])
        ctx.save_for_backward(qkv, p, o)
        ctx.H = H
        return o.transpose(1, 2).reshape(B, N, H * 64)

    @staticmethod
    def backward(ctx, g):
        qkv, p, o = ctx.saved_tensors
        B, N, _ = qkv.shape
        H = ctx.H
        t = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        qq, k, v = t[0], t[1], t[2]
        do = bf(g).reshape(B, N, H, 64).transpose(1, 2)
        pb = bf(p)
        dp = do @ v.transpose(-2, -1)
        delta = (do * o).sum(-1, keepdim=True) if N <= 192 else (p * dp).sum(-1, keepdim=True)
        ds = bf(p * (dp - delta) * 0.125)
        d = torch.stack([bf(ds @ k), bf(ds.transpose(-2, -1) @ qq), bf(pb.transpose(-2, -1) @ do)])      # [3, B, H, N, 64]
        return d.permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * 64), None, None


# ------------------------------------------------------------------------------------------ arena
def dims_of(**kw):
    d = dict(proj=128, dtype=0, exact=1, Pp=0, n_types=0, img_type=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def arena_specs(dims, lay):
    """[(state-dict name, element offset, shape)] of the encoder arena: names and offsets of runtime.param_specs on rmcl_param_layout's
    offsets, shapes for these dims (mlp need not be a multiple of D, the position table has Pp + 1 rows, the patch weight is [D, patch_k])."""
    from fractions import Fraction
    from rmcl_amd.runtime import param_specs
    cfg = dict(hidden_size=dims.D, patch_size=1, image_size=1, mlp_ratio=Fraction(dims.mlp, dims.D), vocab_size=dims.vocab, max_text_len=dims.L,
               num_layers=dims.layers, loss_names={"nlvr2": 1} if dims.n_types == 3 else {})
    out = []
    for name, off, shape in param_specs(cfg, lay):
        if name == "transformer.pos_embed":
            shape = (1, (dims.Pp or dims.P) + 1, dims.D)
        elif name == "transformer.patch_embed.proj.weight":
            shape = (dims.D, dims.patch_k)
        elif name == "moco_head.projector.3.weight":
            shape = (dims.proj, dims.D)
        out.append((name, int(off), tuple(int(v) for v in shape)))
    return out


def numel(shape):
    n = 1
    for v in shape:
        n *= v
    return n


def views(arena, specs):
    return {name: arena[off:off + numel(shape)].view(shape) for name, off, shape in specs}


def init_arena(specs, total, seed):
    """Weights as oracle.init_params scales them: N(0, 0.02), LayerNorm weights 1 + N(0, 0.05); the gaps between slots stay zero."""
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(total, dtype=torch.float32)
    for name, off, shape in specs:
        t = torch.randn(numel(shape), generator=g) * 0.02
        if name.endswith(LN_SUFFIXES):
            t = 1.0 + 2.5 * t
        a[off:off + t.numel()] = t
    return a


def pack(p, specs, total):
    a = torch.zeros(total, dtype=next(iter(p.values())).dtype)
    for name, off, shape in specs:
        a[off:off + numel(shape)] = p[name].reshape(-1)
    return a


# ------------------------------------------------------------------------------------------ the pass
def _pos_rows(pos_img, ragged, B, P, D):
    """[B, 1 + P, D] position rows: the shared table, or per sample the G0 x G0 table resized to (h, w) at the selected patches (0 on pads)."""
    if ragged is None:
        return pos_img[:1 + P][None].expand(B, -1, -1)
    G0, gw = ragged["G0"], ragged["gw"]
    rows = []
    for b in range(B):
        h, w = (int(v) for v in ragged["hw"][b])
        tab = O.resize_pos_embed(pos_img[1:1 + G0 * G0], G0, h, w)                 # [h, w, D]
        r = [pos_img[0]]
        for k in range(P):
            if k < int(ragged["counts"][b]):
                pi = int(ragged["sel"][b, k])
                r.append(tab[pi // gw, pi % gw])
            else:
                r.append(torch.zeros(D, dtype=pos_img.dtype))
        rows.append(torch.stack(r))
    return torch.stack(rows)


def _fold_linear(x, ctr, gamma, beta, W32, bias, eps):
    z = x - ctr[..., None]
    mu = z.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((z - mu) ** 2).mean(-1, keepdim=True) + eps)
    Wf = bf(W32 * gamma)
    return rstd * (bf(z) @ Wf.t() - mu * Wf.sum(1)) + (W32 @ beta + bias)


def _model_block(p, b, x, mask, H, drop, fold, ctr_prev, tail=False):
    """One block with the roundings of the docstring.  Returns (x_out, the LayerNorm-2 row means: the next layer's fold centre).
    tail: the block behind its attention in fp32 on the master weights (the cls-only tail)."""
    d = drop or {}
    W = lambda n: p[b + n] + (bf(p[b + n]) - p[b + n]).detach()
    m1 = x.mean(-1)
    ln1 = q(O.layer_norm(x, p[b + "norm1.weight"], p[b + "norm1.bias"], 1e-6))
    y = ln1 @ W("attn.qkv.weight").t() + p[b + "attn.qkv.bias"]
    if fold and ctr_prev is not None:
        yf = _fold_linear(x, ctr_prev, p[b + "norm1.weight"], p[b + "norm1.bias"], p[b + "attn.qkv.weight"], p[b + "attn.qkv.bias"], 1e-6)
        y = y + (yf - y).detach()
    ao = _AttnModel.apply(q(y), mask, H)
    if tail:
        a = ao @ p[b + "attn.proj.weight"].t() + p[b + "attn.proj.bias"]
        x_mid = x + (a * d["proj"] if "proj" in d else a)
        ln2 = O.layer_norm(x_mid, p[b + "norm2.weight"], p[b + "norm2.bias"], 1e-6)
        h = O.gelu_erf(ln2 @ p[b + "mlp.fc1.weight"].t() + p[b + "mlp.fc1.bias"])
        o = (h * d["hidden"] if "hidden" in d else h) @ p[b + "mlp.fc2.weight"].t() + p[b + "mlp.fc2.bias"]
        return x_mid + (o * d["fc2"] if "fc2" in d else o), x_mid.mean(-1).detach()
    a = qg(ao @ W("attn.proj.weight").t() + p[b + "attn.proj.bias"])
    x_mid = x + (a * d["proj"] if "proj" in d else a)
    m2 = x_mid.mean(-1)
    ln2 = q(O.layer_norm(x_mid, p[b + "norm2.weight"], p[b + "norm2.bias"], 1e-6))
    pre = ln2 @ W("mlp.fc1.weight").t() + p[b + "mlp.fc1.bias"]
    if fold:
        pf = _fold_linear(x_mid, m1.detach(), p[b + "norm2.weight"], p[b + "norm2.bias"], p[b + "mlp.fc1.weight"], p[b + "mlp.fc1.bias"], 1e-6)
        pre = pre + (pf - pre).detach()
    h = _GeluStash.apply(qg(pre))
    h = qf(h * d["hidden"] if "hidden" in d else h)
    o = qg(h @ W("mlp.fc2.weight").t() + p[b + "mlp.fc2.bias"])
    return x_mid + (o * d["fc2"] if "fc2" in d else o), m2.detach()


def encoder_ref(arena, specs, dims, text_ids, text_mask, patches, ragged=None, replaced=None, mask_token=None, drop=None, img_type=None,
                img_of=None, model=False, fold=False, tail=False, word_embeds=None, parts=None):
    """xn [B, N, D] and co_mask [B, N] (int32) of the pass.  patches [Bi * P, patch_k] (bf16 values on a bf16 arm); ragged: dict(sel, counts, hw,
    gw, G0) of CPU tensors; replaced [Bi, P] with mask_token = the NAME of the [D] arena slot that holds the mask token (the _mpp forms); drop: {"text", "image", layer: {"proj", "hidden", "fc2"}}
    scale masks; img_type: rmcl_dims.img_type (default dims.img_type); img_of [B]: the rank pass - the Bi images are a cache and sequence b
    takes image img_of[b] (outside [0, Bi): zero image rows, zero image mask).  parts (a dict): receives "pe" (the patch rows that get dpe) and
    "visual" ([Bi, 1 + P, D] without the token type: rmcl_visual_embed's output) and "visual_mask"."""
    p = views(arena, specs)
    dt = arena.dtype
    D, P, Lt, H = dims.D, dims.P, dims.L, dims.H
    drop = drop or {}
    img_type = dims.img_type if img_type is None else img_type
    Bi = patches.shape[0] // P
    # text rows: BertEmbeddings (word + position + type 0, LayerNorm 1e-12), its dropout, then the ViLT token type 0 - fp32 in every arm
    te = O.text_embed(p, "", text_ids, word_embeds)
    if "text" in drop:
        te = te * drop["text"]
    te = te + p["token_type_embeddings.weight"][0]
    # image rows
    Wp = p["transformer.patch_embed.proj.weight"]
    if model:
        Wp = Wp + (bf(Wp) - Wp).detach()
    pe = patches @ Wp.t() + p["transformer.patch_embed.proj.bias"]
    if model:
        pe = qg(pe)
    pe = pe.view(Bi, P, D)
    if replaced is not None:
        pe = torch.where(replaced.bool()[:, :, None], p[mask_token].view(1, 1, D).expand(Bi, P, D), pe)
    pos = _pos_rows(p["transformer.pos_embed"][0], ragged, Bi, P, D)
    ie = torch.cat([p["transformer.cls_token"].view(1, 1, D).expand(Bi, 1, D), pe], dim=1) + pos
    pp = dims.patch_k // 3
    im = torch.cat([torch.ones(Bi, 1, dtype=torch.int32),
                    (patches.detach().view(Bi, P, 3, pp)[:, :, :, 0].sum(-1) != 0).to(torch.int32)], dim=1)
    if parts is not None:
        parts["visual"], parts["visual_mask"] = ie, im
    if "image" in drop:
        ie = ie * drop["image"]
    vt = p["token_type_embeddings.weight"]
    if img_type == -1:
        ie = ie + torch.stack([vt[1 + (b & 1)] for b in range(Bi)])[:, None]
    else:
        ie = ie + vt[2 if img_type == 2 else 1]
    if img_of is not None:
        ok = [0 <= int(i) < Bi for i in img_of]
        ie = torch.stack([ie[int(i)] if o else torch.zeros(1 + P, D, dtype=dt) for i, o in zip(img_of, ok)])
        im = torch.stack([im[int(i)] if o else torch.zeros(1 + P, dtype=torch.int32) for i, o in zip(img_of, ok)])
    x = torch.cat([te, ie], dim=1)
    co = torch.cat([(text_mask != 0).to(torch.int32), im], dim=1)
    ctr = None
    for l in range(dims.layers):
        b = f"transformer.blocks.{l}."
        if model:
            x, ctr = _model_block(p, b, x, co, H, drop.get(l), fold, ctr, tail and l + 1 == dims.layers)
        else:
            x = O.block(p, b, x, co, H, drop.get(l))
    return O.layer_norm(x, p["transformer.norm.weight"], p["transformer.norm.bias"], 1e-6), co


def grads(arena32, specs, dims, text_ids, text_mask, patches, dxn, dtype, model=False, **kw):
    """Forward + autograd of sum(xn * dxn) in `dtype`.  Returns dict(xn, co, dpatches [Bi * P, patch_k], dtext [B * L, D] - the gradient of the
    word-embedding output -, G = the gradient arena); on the model the data gradient is rounded to bf16 like the kernel's dpatches."""
    a = arena32.detach().to(dtype).clone().requires_grad_(True)
    pt = patches.detach().to(dtype).clone().requires_grad_(True)
    if kw.get("drop"):
        cv = lambda v: {k: cv(t) for k, t in v.items()} if isinstance(v, dict) else v.to(dtype)
        kw["drop"] = cv(kw["drop"])
    we = F.embedding(text_ids, views(a, specs)["text_embeddings.word_embeddings.weight"], padding_idx=0)
    we.retain_grad()
    xn, co = encoder_ref(a, specs, dims, text_ids, text_mask, pt, model=model, word_embeds=we, **kw)
    out = {"xn": xn.detach(), "co": co}
    if dxn is not None:
        (xn * dxn.to(dtype).view_as(xn)).sum().backward()
        out.update(dpatches=bf(pt.grad) if model else pt.grad, dtext=we.grad.reshape(-1, dims.D), G=a.grad)
    return out
