"""Device runtime under the ViLTransformerSS mirror: flat parameter arenas in HBM, per-batch
activation stashes / workspaces, and thin wrappers over the C ABI (include/rmcl.h).

Data layout in HBM (DESIGN.md "Data layout"):
  * q32 / k32     : fp32 parameter arenas (query / momentum), offsets from rmcl_param_layout();
                    the momentum update, AdamW and the gradient all-reduce are single passes
                    over these flat buffers instead of 161 per-tensor ops.
  * q_lp / k_lp   : bf16 shadows of the GEMM weights (bf16 mode only).
  * g32           : fp32 gradient arena, same offsets; the backward kernels accumulate into it.
  * images are converted ONCE per step to patch rows [B*144, 3072] (the K-order of the
    patch-embedding GEMM); delta, the PGD gradient and the attacked view stay in that layout.
torch is used for allocation, streams and torch.distributed only.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Tuple

import torch

from . import _lib as L
from ._lib import lib, check, P, I64, F


def stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def is_nlvr2(cfg: dict) -> bool:
    """NLVR2 fine-tuning (loss_names nlvr2 / nlvr2_attacked): a 3-row token_type_embeddings and the nlvr2_classifier head."""
    ln = cfg.get("loss_names", {})
    return ln.get("nlvr2", 0) > 0 or ln.get("nlvr2_attacked", 0) > 0


def is_irtr(cfg: dict) -> bool:
    """IRTR fine-tuning (loss_names irtr): rank_output = row 1 of the ITM head (vilt_module.py:233-239)."""
    return cfg.get("loss_names", {}).get("irtr", 0) > 0


def irtr_alias_specs(cfg: dict, lay: L.Layout) -> List[Tuple[str, int, Tuple[int, ...]]]:
    """rank_output.weight / .bias of an IRTR model: VIEWS of row 1 of the ITM head's slots (vilt_module.py:233-236) - no arena space of
    their own.  Empty for every other model."""
    if not is_irtr(cfg):
        return []
    D = int(cfg["hidden_size"])
    return [("rank_output.weight", int(lay.itm_w) + D, (1, D)), ("rank_output.bias", int(lay.itm_b) + 1, (1,))]


def make_dims(cfg: dict, B: int, dtype: int, exact: bool, P: int = None) -> L.Dims:
    """P: image patches per sample in this pass (default: the full grid); the position table always has the full grid.
    n_types = 3 for an NLVR2 model (include/rmcl.h rmcl_dims); img_type starts at 0 (row 1) and is set per pass."""
    ps = cfg["patch_size"]
    g = cfg["image_size"] // ps
    return L.Dims(B=B, L=cfg["max_text_len"], P=g * g if P is None else P, D=cfg["hidden_size"], H=cfg["num_heads"],
                  layers=cfg["num_layers"], mlp=cfg["hidden_size"] * cfg["mlp_ratio"], patch_k=3 * ps * ps,
                  proj=128, vocab=cfg["vocab_size"], dtype=dtype, exact=int(exact), Pp=g * g, n_types=3 if is_nlvr2(cfg) else 0,
                  img_type=0)


def param_specs(cfg: dict, lay: L.Layout) -> List[Tuple[str, int, Tuple[int, ...]]]:
    """(reference state-dict name, arena element offset, shape) for every query-side parameter."""
    D = cfg["hidden_size"]
    ps = cfg["patch_size"]
    g = cfg["image_size"] // ps
    Hm = D * cfg["mlp_ratio"]
    s = [
        ("text_embeddings.word_embeddings.weight", lay.word, (cfg["vocab_size"], D)),
        ("text_embeddings.position_embeddings.weight", lay.pos, (cfg["max_text_len"], D)),
        ("text_embeddings.token_type_embeddings.weight", lay.btype, (2, D)),
        ("text_embeddings.LayerNorm.weight", lay.eln_w, (D,)),
        ("text_embeddings.LayerNorm.bias", lay.eln_b, (D,)),
        ("token_type_embeddings.weight", lay.vtype, (3 if is_nlvr2(cfg) else 2, D)),
        ("transformer.cls_token", lay.cls, (1, 1, D)),
        ("transformer.pos_embed", lay.pos_img, (1, g * g + 1, D)),
        ("transformer.patch_embed.proj.weight", lay.patch_w, (D, 3, ps, ps)),
        ("transformer.patch_embed.proj.bias", lay.patch_b, (D,)),
    ]
    for i in range(cfg["num_layers"]):
        b = lay.layer0 + i * lay.layer_stride
        n = f"transformer.blocks.{i}."
        s += [
            (n + "norm1.weight", b + lay.ln1_w, (D,)), (n + "norm1.bias", b + lay.ln1_b, (D,)),
            (n + "attn.qkv.weight", b + lay.qkv_w, (3 * D, D)), (n + "attn.qkv.bias", b + lay.qkv_b, (3 * D,)),
            (n + "attn.proj.weight", b + lay.proj_w, (D, D)), (n + "attn.proj.bias", b + lay.proj_b, (D,)),
            (n + "norm2.weight", b + lay.ln2_w, (D,)), (n + "norm2.bias", b + lay.ln2_b, (D,)),
            (n + "mlp.fc1.weight", b + lay.fc1_w, (Hm, D)), (n + "mlp.fc1.bias", b + lay.fc1_b, (Hm,)),
            (n + "mlp.fc2.weight", b + lay.fc2_w, (D, Hm)), (n + "mlp.fc2.bias", b + lay.fc2_b, (D,)),
        ]
    s += [
        ("transformer.norm.weight", lay.norm_w, (D,)), ("transformer.norm.bias", lay.norm_b, (D,)),
        ("moco_head.projector.0.weight", lay.mh0_w, (D, D)), ("moco_head.projector.0.bias", lay.mh0_b, (D,)),
        ("moco_head.projector.1.weight", lay.mh1_w, (D,)), ("moco_head.projector.1.bias", lay.mh1_b, (D,)),
        ("moco_head.projector.3.weight", lay.mh3_w, (128, D)),
        ("pooler.dense.weight", lay.pool_w, (D, D)), ("pooler.dense.bias", lay.pool_b, (D,)),
        ("itm_score.fc.weight", lay.itm_w, (2, D)), ("itm_score.fc.bias", lay.itm_b, (2,)),
    ]
    return s


EMA_GROUPS = ("text_embeddings", "token_type_embeddings", "transformer", "moco_head")


def _pack(base: int, table):
    """The one arena packer of the optional heads: `table` = [(struct key, state-dict name, shape, element count or None = the
    shape's product)], placed one after the other from element offset `base`, every slot rounded up to 64 elements.  Returns
    (offs {key: element offset}, specs [(name, offset, shape)], elements used)."""
    off, offs, specs = base, {}, []
    for key, name, shape, cnt in table:
        offs[key] = off
        specs.append((name, off, shape))
        if cnt is None:
            cnt = 1
            for v in shape:
                cnt *= v
        off += (cnt + 63) // 64 * 64
    return offs, specs, off - base


def bt_layout(cfg: dict, base: int):
    """BarlowTwinsHead (heads.py:88-107; widths [8192, 8192], 8192 at vilt_module.py:115, config key "barlowtwins_dims")
    appended to the parameter arena at element offset `base`: returns (rmcl_bt_head struct, specs, elements used)."""
    D = cfg["hidden_size"]
    H1, H2, H3 = cfg.get("barlowtwins_dims", (8192, 8192, 8192))
    n = "barlowtwins_head.projector."
    offs, specs, used = _pack(base, [("w1", n + "0.weight", (H1, D), None), ("g1", n + "1.weight", (H1,), None), ("b1", n + "1.bias", (H1,), None),
                                     ("w2", n + "3.weight", (H2, H1), None), ("g2", n + "4.weight", (H2,), None), ("b2", n + "4.bias", (H2,), None),
                                     ("w3", n + "6.weight", (H3, H2), None)])
    return L.BtHead(D=D, H1=H1, H2=H2, H3=H3, **offs), specs, used


class BtBuffers:
    """Per-pass buffers of the Barlow-Twins head: its stash, the projection z, d loss / dz and the distance rows."""

    def __init__(self, eng: "Engine", B: int):
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.device)
        self.B = B
        self.stash = f32(int(lib.rmcl_bt_stash_floats(C.byref(eng.bt), B)))
        self.z = f32(B, eng.bt.H3)
        self.dz = f32(B, eng.bt.H3)
        self.dcls = f32(B, eng.bt.D)
        self.rows = f32(B, 3)
        self.loss2 = f32(2)


def _classifier_layout(prefix: str, D: int, H: int, N: int, ldl: int, base: int):
    """Linear(D, H) - LayerNorm(H) - GELU - Linear(H, N) under the state-dict prefix `prefix` (the shape of vqa_classifier and
    nlvr2_classifier) at element offset `base`: (rmcl_vqa_head struct, specs, elements used).  The last weight keeps ldl rows in
    the arena (ldl = the logits pitch, a multiple of 64): rows N..ldl-1 stay zero (no gradient reaches them, AdamW leaves a zero
    parameter with a zero gradient at zero), so the data gradient dz W3 runs on the padded width."""
    n = prefix
    offs, specs, used = _pack(base, [("w0", n + "0.weight", (H, D), H * D), ("b0", n + "0.bias", (H,), H), ("g1", n + "1.weight", (H,), H),
                                     ("b1", n + "1.bias", (H,), H), ("w3", n + "3.weight", (N, H), ldl * H), ("b3", n + "3.bias", (N,), N)])
    return L.VqaHead(D=D, H=H, N=N, ldl=ldl, **offs), specs, used


def vqa_layout(cfg: dict, base: int):
    """vqa_classifier (vilt_module.py:164-172: Linear(D, 2D) - LayerNorm(2D) - GELU - Linear(2D, vqav2_label_size)) appended to the
    parameter arena at element offset `base`: returns (rmcl_vqa_head struct, specs, elements used); the logits pitch is
    vqav2_label_size rounded up to 64 (_classifier_layout)."""
    D, N = cfg["hidden_size"], int(cfg["vqav2_label_size"])
    return _classifier_layout("vqa_classifier.", D, 2 * D, N, (N + 63) // 64 * 64, base)


def nlvr2_layout(cfg: dict, base: int):
    """nlvr2_classifier (vilt_module.py:193-200: Linear(2D, 2D) - LayerNorm(2D) - GELU - Linear(2D, 2)) appended to the parameter arena
    at element offset `base`: the VQA head struct with D = H = 2 hidden, N = 2 and a logits pitch of 64 (include/rmcl.h).  Returns
    (rmcl_vqa_head struct, specs, elements used).  As for vqa_layout, the last weight keeps ldl rows (rows 2..63 stay zero)."""
    D2 = 2 * cfg["hidden_size"]
    return _classifier_layout("nlvr2_classifier.", D2, D2, 2, 64, base)


class ClassifierBuffers:
    """What the per-pass buffers of the VQA and the NLVR2 head share (both run the rmcl_vqa_head kernels on the struct `h`): the
    stash, the pitched logits and dz, the cls gradient, the row outputs of the loss (`rows_shape`) and the per-row argmax."""

    def __init__(self, eng: "Engine", h, B: int, rows_shape):
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.device)
        self.B = B
        self.stash = f32(int(lib.rmcl_vqa_stash_floats(C.byref(h), B)))
        self.logits_p = f32(B, h.ldl)
        self.logits = self.logits_p[:, : h.N]                  # the public [B, N] view
        self.dz = f32(B, h.ldl)
        self.dcls = f32(B, h.D)                                # (NLVR2: [B, 2 hidden] = the pair pass's [2B, hidden] cls gradient)
        self.rows = f32(*rows_shape)
        self.argmax = torch.empty(B, dtype=torch.int32, device=eng.device)


class VqaBuffers(ClassifierBuffers):
    """Per-pass buffers of the VQA head: its stash, the pitched logits and dz, the row outputs, and the label / score tables of the
    batch (one pinned host buffer, one asynchronous copy: ``Engine.vqa_targets``)."""

    def __init__(self, eng: "Engine", B: int):
        super().__init__(eng, eng.vqa, B, (B, 2))
        self.loss2 = torch.empty(2, dtype=torch.float32, device=eng.device)
        self.A = 0
        self.tab = None                                         # device [2, B, A] int32: labels, then the scores' bits
        self.labels = self.scores = None
        self._host = None


class Nlvr2Buffers(ClassifierBuffers):
    """Per-pass buffers of the NLVR2 head (B = pairs): its stash, the pitched logits and dz, the CE row outputs and the labels."""

    def __init__(self, eng: "Engine", B: int):
        super().__init__(eng, eng.nlvr2, B, (B,))
        self.stats = torch.empty(3, dtype=torch.float32, device=eng.device)
        self.labels = torch.empty(B, dtype=torch.int32, device=eng.device)


def _transform_rows(n: str, D: int):
    """the four `_pack` rows of a prediction head's BertPredictionHeadTransform (heads.py: dense, LayerNorm) under the module name `n`"""
    return [("tw", n + "transform.dense.weight", (D, D), None), ("tb", n + "transform.dense.bias", (D,), None),
            ("lg", n + "transform.LayerNorm.weight", (D,), None), ("lb", n + "transform.LayerNorm.bias", (D,), None)]


def mlm_layout(cfg: dict, base: int):
    """mlm_score (heads.py:183-195, built WITHOUT a tied weight at vilt_module.py:56: decoder.weight [vocab, D] is a parameter of its
    own) appended to the parameter arena at element offset `base`: returns (rmcl_mlm_head struct, specs, elements used)."""
    D, V = int(cfg["hidden_size"]), int(cfg["vocab_size"])
    n = "mlm_score."
    offs, specs, used = _pack(base, _transform_rows(n, D) + [("dw", n + "decoder.weight", (V, D), None), ("db", n + "bias", (V,), None)])
    return L.MlmHead(D=D, V=V, **offs), specs, used


class CompactedHeadBuffers:
    """What the per-pass buffers of the prediction heads (MLM, MPP) share: the compaction of at most `max_rows` rows (row list, `groups`
    labels per row, `ncount` device-side counts), the per-row outputs and the workspace the forward leaves for the backward.  ``cap``:
    `max_rows` rounded up to 128; ``rows``: launch extent for the bound batch (``bind_rows``)."""

    def __init__(self, eng: "Engine", max_rows: int, groups: tuple, ncount: int, ws_floats, head):
        self.cap = (max_rows + 127) // 128 * 128
        i32 = lambda *n: torch.empty(*n, dtype=torch.int32, device=eng.device)
        f32 = lambda *n: torch.empty(*n, dtype=torch.float32, device=eng.device)
        self.idx, self.lab, self.count = i32(self.cap), i32(self.cap, *groups), i32(ncount)
        self.lse, self.rowloss, self.argmax = f32(self.cap, *groups), f32(self.cap), i32(self.cap, *groups)
        self.ws = f32(int(ws_floats(C.byref(head), self.cap)))
        self.rows = self.cap

    def bind_rows(self, n: int, all_rows: bool):
        """the launch extent for a batch with (at most) n listed rows, known on the host: a multiple of 128, at least 128; all_rows: cap"""
        self.rows = self.cap if all_rows else min(self.cap, max(128, (n + 127) // 128 * 128))


class MlmBuffers(CompactedHeadBuffers):
    """Per-(batch, tag) buffers of the MLM head for M = B x L text positions (``rows`` >= the number of labelled rows)."""

    def __init__(self, eng: "Engine", B: int):
        self.B, self.L = B, int(eng.cfg["max_text_len"])
        self.M = B * self.L
        super().__init__(eng, self.M, (), 1, lib.rmcl_mlm_ws_floats, eng.mlm)
        self.labels = None                                      # the bound [B, L] int64 labels on the device


def mpp_layout(cfg: dict, base: int):
    """transformer.mask_token (vision_transformer.py: nn.Parameter(zeros(1, 1, D))) and mpp_score (heads.MPPHead, heads.py:198-207:
    BertPredictionHeadTransform + Linear(D, 768)) appended to the parameter arena at element offset `base`: returns (rmcl_mpp_head
    struct, specs, elements used)."""
    D = int(cfg["hidden_size"])
    n = "mpp_score."
    offs, specs, used = _pack(base, [("mt", "transformer.mask_token", (1, 1, D), None)] + _transform_rows(n, D) +
                              [("dw", n + "decoder.weight", (768, D), None), ("db", n + "decoder.bias", (768,), None)])
    return L.MppHead(D=D, reserved=0, **offs), specs, used


def mpp_draw_masks(B: int, G: int):
    """The two mask draws of VisionTransformer.mask_tokens (vision_transformer.py:547-554) over the full patch grid [B, G], on torch's
    global CPU generator and in the reference's order: masked ~ Bernoulli(0.15), then replaced = Bernoulli(0.8) & masked.  Under the same
    torch.manual_seed the draws coincide with the reference's.  Returns two bool tensors on the host."""
    masked = torch.bernoulli(torch.full((B, G), 0.15)).bool()
    replaced = torch.bernoulli(torch.full((B, G), 0.8)).bool() & masked
    return masked, replaced


class MppBuffers(CompactedHeadBuffers):
    """Per-(batch, tag, image length) buffers of the MPP head for B x P image slots: the slot labels and the masks gathered through the
    batch's patch selection, then the compacted set (three labels per row; ``rows`` >= the host-known number of masked slots)."""

    def __init__(self, eng: "Engine", B: int, Pn: int):
        self.B, self.P = B, Pn
        # (all image rows, the cls rows included: the dense-logits pass)
        super().__init__(eng, B * (Pn + 1), (3,), 2, lib.rmcl_mpp_ws_floats, eng.mpp)
        self.labels = torch.empty(B, Pn, 3, dtype=torch.int32, device=eng.device)
        self.masked = self.replaced = None                      # [B, P] int32 on the device, of the bound batch
        self.n_masked = self.cap                                # host-known bound of the listed rows (mpp_labels_masks)


class PassBuffers:
    """Everything sized by the per-GPU batch B (allocated once, reused every step)."""

    def __init__(self, eng: "Engine", B: int, dtype=None, P=None, lane_of: "PassBuffers" = None, lane: int = 0):
        """lane_of / lane: these buffers are LANE `lane` of `lane_of` (samples [lane * B, (lane + 1) * B) of its batch): everything that is
        laid out per sample is a row-range VIEW of the parent's tensor, only the scratch of a pass (workspace, stashes, InfoNCE
        workspace, loss ring) is the lane's own - see Engine.lanes."""
        dev = eng.device
        self.dtype = eng.dtype if dtype is None else dtype       # arithmetic of the passes run through these buffers
        d = eng.dims(B, self.dtype, P)
        if lane_of is not None:
            self._init_lane(eng, d, lane_of, lane)
            return
        self.geom = None                # RaggedGeometry of a zero-padded batch (None: full-size images, dense patches)
        self.ragged = None              # the rmcl_ragged struct handed to the encoder passes (own pos_tok / dpos_tok scratch)
        self.B = B
        self.d = d
        N = d.L + 1 + d.P
        M = B * N
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self._init_scratch(eng, d, full_stash=True)
        self.co_mask = torch.empty(B, N, dtype=torch.int32, device=dev)
        self.xn = f32(M, d.D)
        self.patches32 = f32(B * d.P, d.patch_k)
        tdt = torch.float32 if self.dtype == L.F32 else torch.bfloat16
        self.patchesT = torch.empty(B * d.P, d.patch_k, dtype=tdt, device=dev)
        self.patchesT_full = torch.empty(B * d.P, d.patch_k, dtype=tdt, device=dev)
        self.gpatch = torch.empty(B * d.P, d.patch_k, dtype=tdt, device=dev)
        self.delta = f32(B * d.P, d.patch_k)
        self.delta_prev = f32(B * d.P, d.patch_k)
        self.amax = torch.empty(64 * B, dtype=torch.int32, device=dev)      # include/rmcl.h rmcl_pgd_step: 64 partial maxima per sample
        self.ball = torch.empty(int(lib.rmcl_pgd_ball_scratch_bytes(B)), dtype=torch.uint8, device=dev)   # rmcl_pgd_step_ball's partials
        self.cls = f32(B, d.D)
        self.q = f32(B, d.proj)
        self.k = f32(B, d.proj)
        self.dq = f32(B, d.proj)
        self.dcls = f32(B, d.D)
        self.rows = f32(B, 10)

    def _init_scratch(self, eng: "Engine", d, full_stash: bool):
        """The scratch of one pass, owned by whole-batch buffers and lanes alike: workspace, stashes, loss ring, InfoNCE workspace, and
        the per-step defaults (text tensors, position rows, dropout seeds, tail flags)."""
        dev = eng.device
        u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)
        self.workspace = u8(lib.rmcl_workspace_bytes(C.byref(d)))
        self.stash_full = u8(lib.rmcl_stash_bytes(C.byref(d), L.MODE_FULL)) if full_stash else None   # lanes run the data-gradient passes only
        self.stash_data = u8(lib.rmcl_stash_bytes(C.byref(d), L.MODE_DATA))
        self.hstash_q = u8(lib.rmcl_heads_stash_bytes(C.byref(d)))
        self.hstash_k = u8(lib.rmcl_heads_stash_bytes(C.byref(d)))
        self.loss_ring = torch.zeros(32, dtype=torch.float32, device=dev)    # zeroed scalars for the kernels that ACCUMULATE a loss / norm:
        self.loss_i = 0                                                      # one fill per 32 uses instead of one per use (zero_scalar)
        self.loss_sum = self.loss_ring[0:1]
        self.nce_ws = u8(lib.rmcl_infonce_ws_bytes(d.B, I64(eng.num_negative)))
        self.text_ids = None
        self.text_mask = None
        self.pos_tok = self.dpos_tok = None      # per-sample position rows of a zero-padded batch and their gradient (lazy)
        self.drop = {L.MODE_INFER: (0, 0.0), L.MODE_DATA: (0, 0.0), L.MODE_FULL: (0, 0.0)}
        self.tail = {}                           # mode -> the last forward in that mode used the cls-only tail

    def _init_lane(self, eng: "Engine", d, par: "PassBuffers", lane: int):
        B = d.B
        N = d.L + 1 + d.P
        rows = lambda t, per: t[lane * B * per:(lane + 1) * B * per]
        self.geom = self.ragged = None
        self.B, self.d, self.lane, self.parent = B, d, lane, par
        self._init_scratch(eng, d, full_stash=False)
        self.co_mask = rows(par.co_mask, 1)
        self.xn = rows(par.xn, N)
        self.patches32, self.patchesT, self.patchesT_full = rows(par.patches32, d.P), rows(par.patchesT, d.P), rows(par.patchesT_full, d.P)
        self.gpatch, self.delta, self.delta_prev = rows(par.gpatch, d.P), rows(par.delta, d.P), rows(par.delta_prev, d.P)
        self.amax = rows(par.amax, 64)
        # (the threat-model scratch is laid out per array, not per sample: a lane has its own 1 280 bytes per sample)
        self.ball = torch.empty(int(lib.rmcl_pgd_ball_scratch_bytes(B)), dtype=torch.uint8, device=eng.device)
        self.cls, self.q, self.k, self.dq, self.dcls, self.rows = (rows(t, 1) for t in (par.cls, par.q, par.k, par.dq, par.dcls, par.rows))


class RankPass:
    """Buffers of the cached rank pass (inference only: a workspace, the mask, xn, the pooled cls rows).  ONE set,
    grown to the largest (sequences, patches) asked for and viewed at every smaller shape, so tiles of any padded length share it
    (DESIGN.md "IRTR fine-tuning and recall")."""

    def __init__(self, eng: "Engine"):
        self.eng = eng
        self.geom = self.ragged = None
        self._ws = self._hst = self._co = self._xn = self._cls = None

    def _grow(self, name, n, dtype):
        t = getattr(self, name)
        if t is None or t.numel() < n:
            t = torch.empty(int(n), dtype=dtype, device=self.eng.device)
            setattr(self, name, t)
        return t

    def shape(self, B: int, P: int) -> "RankPass":
        eng = self.eng
        d = eng.dims(B, None, P)
        N = d.L + 1 + d.P
        self.B, self.d, self.dtype = B, d, eng.dtype
        self.workspace = self._grow("_ws", lib.rmcl_workspace_bytes(C.byref(d)), torch.uint8)
        self.hstash_q = self._grow("_hst", lib.rmcl_heads_stash_bytes(C.byref(d)), torch.uint8)
        self.co_mask = self._grow("_co", B * N, torch.int32)[: B * N].view(B, N)
        self.xn = self._grow("_xn", B * N * d.D, torch.float32)[: B * N * d.D].view(B * N, d.D)
        self.cls = self._grow("_cls", B * d.D, torch.float32)[: B * d.D].view(B, d.D)
        return self


class RaggedGeometry:
    """Patch selection of a zero-padded batch [B,3,Hmax,Wmax] (VisionTransformer.visual_embed, vision_transformer.py:559-651):
    sel [B, cap] int32 flat patch indices (valid patches row-major, then pads), counts [B], hw [B,2] = (x_h, x_w), n slots."""

    def __init__(self, sel, counts, hw, n, gh, gw, shape):
        self.sel, self.counts, self.hw, self.n, self.gh, self.gw, self.shape = sel, counts, hw, n, gh, gw, shape

    def take(self, owner: torch.Tensor) -> "RaggedGeometry":
        """geometry of the batch [owner[0], owner[1], ...] (candidate sentences of the text attack reuse their sample's image)"""
        return RaggedGeometry(self.sel.index_select(0, owner).contiguous(), self.counts.index_select(0, owner).contiguous(),
                              self.hw.index_select(0, owner).contiguous(), self.n, self.gh, self.gw,
                              (int(owner.numel()),) + tuple(self.shape[1:]))


class Engine:
    def __init__(self, cfg: dict, device, dtype: str = "bf16", exact: bool = False, pgd_dtype=None):
        if not torch.cuda.is_available():
            raise L.RmclError("rmcl_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = {"f32": L.F32, "fp32": L.F32, "bf16": L.BF16}[dtype]
        self.exact = bool(exact) or self.dtype == L.F32
        # precision of the PGD inner loop only: the reference forces fp32 there (attack/pgd_attack_vilt.py:141) while its
        # main forwards run under autocast; "f32" reproduces that split on a bf16 engine (exact fp32 matrix cores: a
        # measurement / parity mode, ~6x slower than bf16 PGD).  None: PGD runs in the engine's dtype.
        self.pgd_dtype = {None: None, "f32": L.F32, "fp32": L.F32, "bf16": None}[pgd_dtype] if self.dtype == L.BF16 else None
        self.num_negative = int(cfg.get("num_negative", 65536))
        # config["long_sequences"] (bool, default False): a bf16 engine runs passes of 257..512 tokens (max_image_len = -1 of the fine-tuning
        # tasks: 384 x 640 gives 240 + 1 + 40 = 281) through the streaming attention kernels (include/rmcl.h RMCL_MODE_STREAM_ATTN) instead
        # of refusing them; every encoder pass of more than 256 tokens then carries the mode bit (stream_bit).
        self.long_sequences = bool(cfg.get("long_sequences", False)) and self.dtype == L.BF16
        self.token_cap = 512 if self.long_sequences else 256       # tokens per sequence on the bf16 path
        # A model that went out of use is freed by the CYCLE collector only (the deferred-backward closures and the optimizer tie module,
        # engine and pass buffers into cycles), and Python runs that collector by object counts, not by device bytes: a process that builds
        # model after model (a test session) was seen holding 130 - 280 GB of dead arenas.  Collect before this engine allocates its own.
        import gc
        gc.collect()
        d0 = self.dims(1)
        self.layout = L.Layout()
        lib.rmcl_param_layout(C.byref(d0), C.byref(self.layout))
        lay = self.layout
        z = lambda n, dt=torch.float32: torch.zeros(int(n), dtype=dt, device=self.device)
        # optional heads, appended behind the C layout's tensors in this fixed order, so the optimizer, the gradient reduction and the
        # state dict see them as part of the same arena; a model without a head keeps its arena size and specs:
        #   bt    Barlow-Twins head (loss_names["barlowtwins"] > 0)
        #   vqa   VQA classifier (loss_names["vqa"] / ["vqa_attacked"] > 0)
        #   nlvr2 NLVR2 classifier (loss_names["nlvr2"] / ["nlvr2_attacked"] > 0); the 3-row token-type table of these models is part
        #         of the C layout (rmcl_dims.n_types = 3, make_dims)
        #   mlm   MLM head (loss_names["mlm"] > 0)
        #   mpp   transformer.mask_token + MPP head (loss_names["mpp"] > 0)
        ln = cfg.get("loss_names", {})
        extra = 0
        for attr, present, layout_of in (("bt", ln.get("barlowtwins", 0) > 0, bt_layout),
                                         ("vqa", ln.get("vqa", 0) > 0 or ln.get("vqa_attacked", 0) > 0, vqa_layout),
                                         ("nlvr2", is_nlvr2(cfg), nlvr2_layout), ("mlm", ln.get("mlm", 0) > 0, mlm_layout),
                                         ("mpp", ln.get("mpp", 0) > 0, mpp_layout)):
            head, specs, used = layout_of(cfg, int(lay.total) + extra) if present else (None, [], 0)
            setattr(self, attr, head)
            setattr(self, attr + "_specs", specs)
            extra += used
        self._head_bufs = {}                                    # (buffer class, B, tag) -> per-pass buffers of a head (_head_buffers)
        if self.bt is not None:
            H = self.bt
            self.bt_running = torch.cat([torch.zeros(H.H1), torch.ones(H.H1), torch.zeros(H.H2), torch.ones(H.H2), torch.zeros(H.H3),
                                         torch.ones(H.H3)]).to(self.device)      # [mean1, var1, mean2, var2, mean3, var3]
            self.bt_tracked = torch.zeros(3, dtype=torch.int64, device=self.device)
            self.bt_corr = torch.empty(H.H3, H.H3, dtype=torch.float32, device=self.device)
            self.bt_ws = torch.empty(int(lib.rmcl_bt_loss_ws_floats(H.H3)), dtype=torch.float32, device=self.device)
        if self.mlm is not None:
            self.mlm_wT = None                                  # decoder.weight^T in the operand type (rmcl_mlm_weight_transpose)
            self.mlm_wt_stale = True
        # IRTR (loss_names["irtr"] > 0): rank_output.weight / .bias ARE row 1 of the ITM head's slots (vilt_module.py:233-239 makes them
        # views of itm_score.fc): no arena space of their own; `specs` keeps its entries, the aliases are listed apart
        self.irtr = is_irtr(cfg)
        self.alias_specs = irtr_alias_specs(cfg, lay)
        self._rank_pass = None
        self.total = int(lay.total) + extra
        self.q32 = z(self.total)
        self.k32 = z(lay.ema_end)
        self.g32 = z(self.total)
        self.q_lp = z(self.total, torch.bfloat16) if self.dtype == L.BF16 else None
        self.k_lp = z(lay.ema_end, torch.bfloat16) if self.dtype == L.BF16 else None
        # LayerNorm folded into the qkv / fc1 GEMMs of the passes that keep no LayerNorm output (include/rmcl.h rmcl_fold):
        # W' = W * gamma (bf16) + the s / c vectors per arena, re-derived whenever the fp32 masters change
        self.fold = {}
        self.fold_stale = {"q": True, "k": True}
        if self.dtype == L.BF16 and os.environ.get("RMCL_NO_LN_FOLD", "0") != "1":
            nw, ns = lib.rmcl_ln_fold_elems(C.byref(d0), 0), lib.rmcl_ln_fold_elems(C.byref(d0), 1)
            for a in ("q", "k"):
                wf, sc = z(nw, torch.bfloat16), z(ns)
                self.fold[a] = (wf, sc, L.Fold(wf=wf.data_ptr(), sc=sc.data_ptr()))
        # transposed bf16 shadows of the layer weights for the data-gradient GEMMs (include/rmcl.h rmcl_weight_transpose_bf16)
        self.q_lpT = z(lay.total, torch.bfloat16) if (self.dtype == L.BF16 and os.environ.get("RMCL_NO_WT", "0") != "1") else None
        self.lpT_stale = True
        if self.dtype == L.BF16 and self.q_lpT is None:
            check(lib.rmcl_tune_set(15, 0), "tune_set")    # no transposed shadows: the backward cannot read a tiled pre-activation stash
        self.specs = param_specs(cfg, lay) + self.bt_specs + self.vqa_specs + self.nlvr2_specs + self.mlm_specs + self.mpp_specs
        self._bufs: Dict[tuple, PassBuffers] = {}
        self.lp_stale = True
        self.drop_p = float(cfg.get("drop_rate", 0.0))
        self.dropout_on = False            # set by the module per step (self.training)
        self.seed_base = int(cfg.get("seed", 0)) + 1
        self.pass_counter = 0
        self.pass_log = None               # a list here records every encoder pass (tests/test_path_gpu.py: the dropout masks of a whole step)
        self._lut = None                                                   # 256-entry normalisation table of the uint8 feed path
        self.side_stream = torch.cuda.Stream(device=self.device)
        self.dw_stream = torch.cuda.Stream(device=self.device)
        self.comm_stream = torch.cuda.Stream(device=self.device)     # gradient all-reduces (N > 1), gated on backward events
        if os.environ.get("RMCL_NO_DW_STREAM", "0") != "1":          # weight-gradient GEMMs concurrent with the dX chain
            lib.rmcl_set_side_stream(C.c_void_p(self.dw_stream.cuda_stream))
        # stash prefetch of the backward (rmcl_tune_set(12, mask)): on the communication stream, idle outside the gradient reduction
        pf = {"comm": self.comm_stream, "side": self.side_stream, "dw": self.dw_stream}[os.environ.get("RMCL_PREFETCH_STREAM", "comm")]
        lib.rmcl_set_prefetch_stream(C.c_void_p(pf.cuda_stream))

    # ---- geometry ------------------------------------------------------------------------------
    def dims(self, B: int, dtype=None, P=None) -> L.Dims:
        dt = self.dtype if dtype is None else dtype
        return make_dims(self.cfg, B, dt, getattr(self, "exact", False) or dt == L.F32, P)

    def bufs(self, B: int, tag: str = "moco", dtype=None, P=None) -> PassBuffers:
        """Per-(batch size, patches per sample, objective) buffers: each objective keeps its own FULL stash so that several
        task losses of one training_step can be backpropagated after all forwards have run."""
        key = (B, tag) if P is None else (B, tag, P)
        if key not in self._bufs:
            self._bufs[key] = PassBuffers(self, B, dtype, P)
        return self._bufs[key]

    def twin(self, pb: PassBuffers, tag: str, dtype=None, owner: torch.Tensor = None) -> PassBuffers:
        """Buffers of another pass over the SAME images (same patch geometry): the key encoder, another view, the fp32 PGD
        twin; with `owner` the batch [owner[i]] (text-attack candidates).  Shares nothing but the geometry."""
        B = pb.B if owner is None else int(owner.numel())
        geom = pb.geom if (pb.geom is None or owner is None) else pb.geom.take(owner)
        pv = self.bufs(B, tag, dtype, None if pb.geom is None else pb.geom.n)
        self._set_geometry(pv, geom)
        pv.d.img_type = pb.d.img_type                       # (the same images: the same token-type rows)
        return pv

    def _set_geometry(self, pb: PassBuffers, geom):
        pb.geom = geom
        pb.ragged = None
        if geom is not None:
            g0 = self.cfg["image_size"] // self.cfg["patch_size"]
            if pb.pos_tok is None:
                pb.pos_tok = torch.empty(pb.B, pb.d.P + 1, pb.d.D, dtype=torch.float32, device=self.device)
                pb.dpos_tok = torch.empty(pb.B, pb.d.P + 1, pb.d.D, dtype=torch.float32, device=self.device)
            pb.ragged = L.Ragged(sel=geom.sel.data_ptr(), counts=geom.counts.data_ptr(), hw=geom.hw.data_ptr(),
                                 sel_ld=geom.sel.shape[1], gw=geom.gw, G0=g0, pos_tok=pb.pos_tok.data_ptr(),
                                 dpos_tok=pb.dpos_tok.data_ptr())

    @staticmethod
    def _rg(pb: PassBuffers):
        return C.byref(pb.ragged) if pb.ragged is not None else None

    def lanes(self, pb: PassBuffers, n: int = None):
        """The batch of `pb` as n independent half-size passes (or None where that does not apply).  Why: at B = 64 every launch of the
        encoder fills the chip by itself, so all CUs load, run their k-loops and reach their (HBM-bound) epilogues TOGETHER, and most
        launches are one tile per CU - nothing runs under a tile's prologue / epilogue.  Two chains of B / 2 on two HIP streams take
        half the CUs each and drift apart, so one chain's epilogues and attention kernels fall into the other's k-loops
        (tools/two_stream_test.py: 12-layer forward 2.93 ms as one chain, 2.58-2.70 ms as two).  The passes of the PGD loop are
        independent per sample (the loss couples them only through the constant 1 / B), so each lane runs its own K-step loop.
        RMCL_LANES=0 turns this off, RMCL_LANES=1 forces it for any even B (tests); default: even B >= 32, dense full-size images,
        bf16 passes.  Dropout (round 4): every lane's pass draws its own seed (`encoder_forward`), remembered with the lane's stash, so
        forward and backward of a lane agree; the masks of a lane are indexed by the lane's own rows - a different, equally valid draw
        than the one-chain step's (tests hand the materialised per-lane masks to the oracle)."""
        mode = os.environ.get("RMCL_LANES", "auto")
        n = int(os.environ.get("RMCL_LANE_COUNT", "2")) if n is None else n
        if mode == "0" or pb.B % n or pb.geom is not None or pb.dtype != L.BF16 or self.exact:
            return None
        if mode != "1" and pb.B < 32:
            return None
        if pb.d.img_type == -1 and (pb.B // n) % 2:                      # an NLVR2 pair pass is never split inside a pair
            return None
        ls = getattr(pb, "_lanes", None)
        if ls is None or len(ls) != n:
            ls = pb._lanes = [PassBuffers(self, pb.B // n, pb.dtype, None, lane_of=pb, lane=i) for i in range(n)]
        for i, ln in enumerate(ls):                                          # the text tensors are new every step
            ln.d.img_type = pb.d.img_type
            ln.text_ids = pb.text_ids[i * ln.B:(i + 1) * ln.B]
            ln.text_mask = pb.text_mask[i * ln.B:(i + 1) * ln.B]
            ln.k = pb.k[i * ln.B:(i + 1) * ln.B]                             # (pb.k may have been re-pointed: compute_moco_contrastive)
        return ls

    def pgd_bufs(self, pb: PassBuffers) -> PassBuffers:
        """Buffers of the PGD inner loop: `pb` itself, or (pgd_dtype="f32" on a bf16 engine) an fp32 twin that shares the
        batch, the keys and the perturbation buffers with `pb`."""
        if self.pgd_dtype is None or self.pgd_dtype == pb.dtype:
            return pb
        pp = self.twin(pb, "pgd_f32", self.pgd_dtype)
        pp.text_ids, pp.text_mask, pp.patches32 = pb.text_ids, pb.text_mask, pb.patches32
        pp.delta, pp.delta_prev, pp.k = pb.delta, pb.delta_prev, pb.k
        return pp

    def view(self, arena: torch.Tensor, off: int, shape) -> torch.Tensor:
        n = 1
        for s in shape:
            n *= s
        return arena[off:off + n].view(*shape)

    # ---- parameter maintenance -----------------------------------------------------------------
    def refresh_shadows(self):
        """bf16 shadows of the query / momentum weights (after load_state_dict or an optimizer step)."""
        if self.dtype == L.BF16:
            check(lib.rmcl_cast_f32(P(self.q32), P(self.q_lp), L.BF16, I64(self.q32.numel()), stream_ptr()), "cast")
            check(lib.rmcl_cast_f32(P(self.k32), P(self.k_lp), L.BF16, I64(self.k32.numel()), stream_ptr()), "cast")
        self.lp_stale = False
        self.fold_stale = {"q": True, "k": True}
        self.lpT_stale = True
        self.mlm_wt_stale = True

    def weights_T(self):
        """transposed bf16 weight shadows of the query arena (None: the backward reads the weights as stored)"""
        if self.q_lpT is None:
            return None
        if self.lp_stale:
            self.refresh_shadows()
        if self.lpT_stale:
            d0 = self.dims(1)
            check(lib.rmcl_weight_transpose_bf16(C.byref(d0), P(self.q_lp), P(self.q_lpT), stream_ptr()), "weight_transpose")
            self.lpT_stale = False
        return self.q_lpT

    def fold_of(self, key: bool):
        """rmcl_fold of the arena a pass reads (None: separate LayerNorm kernels), refreshed if its masters changed."""
        a = "k" if key else "q"
        if a not in self.fold:
            return None
        wf, sc, st = self.fold[a]
        if self.fold_stale[a]:
            d0 = self.dims(1)
            check(lib.rmcl_ln_fold(C.byref(d0), P(self.k32 if key else self.q32), P(wf), P(sc), stream_ptr()), "ln_fold")
            self.fold_stale[a] = False
        return C.byref(st)

    def ema(self, m: float):
        n = self.layout.ema_end
        check(lib.rmcl_ema_f32(P(self.k32), P(self.q32), P(self.k_lp), F(m), I64(n), stream_ptr()), "ema")
        self.fold_stale["k"] = True

    def zero_grads(self):
        self.g32.zero_()

    # ---- per-step data -------------------------------------------------------------------------
    def patch_geometry(self, img: torch.Tensor, select: torch.Tensor = None, max_image_len=None, check_tokens: bool = True):
        """None for a batch of full-size images (every patch of the image_size x image_size grid valid), else the
        RaggedGeometry of the zero-padded batch.  One device->host copy of B counts (n sizes the launches).
        config["dense_images"] = True skips the check for image_size x image_size inputs (synthetic benchmarks)."""
        B, Cc, Hh, Ww = img.shape
        ps = self.cfg["patch_size"]
        S = self.cfg["image_size"]
        if Cc != 3 or Hh % ps or Ww % ps:
            raise ValueError(f"images must be [B,3,H,W] with H, W multiples of patch_size={ps} (got {tuple(img.shape)}); "
                             "MinMaxResize of the reference rounds both sides to multiples of 32 (transforms/utils.py:5-26)")
        if Hh == S and Ww == S and select is None and self.cfg.get("dense_images", False):
            return None
        gh, gw = Hh // ps, Ww // ps
        if gh * gw > 1024:
            raise ValueError(f"at most 1024 patches per image ({gh}x{gw} given)")
        sel = torch.empty(B, gh * gw, dtype=torch.int32, device=self.device)
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        hw = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        check(lib.rmcl_patch_select(P(img), B, 3, Hh, Ww, ps, P(sel), P(counts), P(hw), stream_ptr()), "patch_select")
        cnt = counts.cpu()
        if Hh == S and Ww == S and select is None and bool((cnt == gh * gw).all()):
            return None
        sel, counts, n = self._cap_selection(sel, counts, cnt, select, max_image_len, check_tokens)
        return RaggedGeometry(sel, counts, hw, n, gh, gw, (B, 3, Hh, Ww))

    def _cap_selection(self, sel: torch.Tensor, counts: torch.Tensor, cnt: torch.Tensor, select, max_image_len=None, check_tokens: bool = True):
        """The image length n of a zero-padded batch and its selection cut to it.  sel [B, G] / counts [B]: the valid-patch lists, both
        on the device or both on the host; cnt: the counts on the HOST.  n = the largest count, capped at max_image_len (default: the
        config's).  `select`: the caller's draw [B, n] replaces sel (parity tests: the reference's); else every sample with more than n
        valid patches keeps a random subset, drawn on the host's generator in sample order.  Returns (sel, counts clamped to n, n)."""
        B = cnt.shape[0]
        n = int(cnt.max())
        mil = self.cfg.get("max_image_len", -1) if max_image_len is None else max_image_len
        if isinstance(mil, int) and mil > 0:
            n = min(n, mil)                                                # vision_transformer.py:602-616
        if check_tokens and n + 1 + self.cfg["max_text_len"] > self.token_cap and self.dtype == L.BF16:
            if self.long_sequences:
                raise self.token_limit_error(n)
            raise NotImplementedError(f"{n} image patches + text exceed the 256-token limit of the fused attention kernels")
        over = []
        if select is not None:
            sel = select.to(sel.device, torch.int32).contiguous()
            assert sel.shape == (B, n), (tuple(sel.shape), (B, n))
        else:
            over = (cnt > n).nonzero().flatten().tolist()
            for b in over:                                                 # more valid patches than max_image_len: the reference
                v = int(cnt[b])                                            # keeps a random subset (multinomial w/o replacement, :633-636)
                keep = torch.multinomial(torch.ones(v).float(), n).to(sel.device)
                sel[b, :n] = sel[b, :v].index_select(0, keep)
        if select is not None or over:                                     # (otherwise no count exceeds n: nothing to clamp, no launch)
            counts = torch.minimum(counts, torch.full_like(counts, n))
        return sel, counts, n

    def _bind(self, text_ids: torch.Tensor, text_mask: torch.Tensor, geom, B: int, tag: str, img_type: int = 0) -> PassBuffers:
        """What every bind ends in: the buffers of (B, tag, image length) with the batch's geometry, token-type row and text.
        img_type 0: token-type row 1 (callers that need another row set it after); -1: the NLVR2 pair pass."""
        pb = self.bufs(B, tag, None, None if geom is None else geom.n)
        self._set_geometry(pb, geom)
        pb.d.img_type = img_type
        pb.text_ids = text_ids.to(self.device, torch.int64).contiguous()
        pb.text_mask = text_mask.to(self.device, torch.int64).contiguous()
        return pb

    def _im2patch(self, img: torch.Tensor, pat: torch.Tensor, geom, B: int, Hh: int, Ww: int, inverse: bool = False):
        """image [B,3,Hh,Ww] -> patch rows `pat` (inverse: patch rows -> image, zero outside the selected patches): every patch of the
        grid (geom None) or the selected ones."""
        ps, name = self.cfg["patch_size"], "patch2im" if inverse else "im2patch"
        if geom is None:
            check(lib.rmcl_im2patch_f32(P(img), P(pat), B, 3, Hh, Ww, ps, int(inverse), stream_ptr()), name)
        else:
            check(lib.rmcl_im2patch_sel(P(img), P(pat), P(geom.sel), P(geom.counts), geom.sel.shape[1], B, geom.n, 3, Hh, Ww, ps,
                                        int(inverse), stream_ptr()), name + "_sel")

    def bind_batch(self, text_ids: torch.Tensor, text_mask: torch.Tensor, image, tag: str = "moco",
                   select: torch.Tensor = None) -> PassBuffers:
        """image: the float batch [B,3,H,W] of ``collate`` - or a ``Uint8Batch`` (``collate_uint8``): the decoded bytes, normalised,
        zero-padded and cut into patch rows by ONE kernel, the patch selection derived from the known extents (no selection
        launch, no device-to-host read of the counts)."""
        if hasattr(image, "tables") and hasattr(image, "data"):                # RawUint8Batch: decoded bytes, MinMaxResize still owed
            image = self.resize_raw(image)
        if hasattr(image, "sizes") and hasattr(image, "data"):
            return self._bind_uint8(text_ids, text_mask, image, tag, select)
        img = image.to(self.device, torch.float32).contiguous()
        B, Cc, Hh, Ww = img.shape
        geom = self.patch_geometry(img, select)
        pb = self._bind(text_ids, text_mask, geom, B, tag)
        self._im2patch(img, pb.patches32, geom, B, Hh, Ww)
        return pb

    @staticmethod
    def _pad_to(img: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """zero-pad a collated batch bottom / right to (H, W), like BaseDataset.collate pads every image of a batch (base_dataset.py:192-206)"""
        if img.shape[2] == H and img.shape[3] == W:
            return img
        return torch.nn.functional.pad(img, (0, W - img.shape[3], 0, H - img.shape[2]))

    def _full_geometry(self, B: int, gh: int, gw: int) -> RaggedGeometry:
        """selection of a batch whose every patch is valid (the ragged form of a full-size image, for a pair with one ragged key)"""
        sel = torch.arange(gh * gw, dtype=torch.int32, device=self.device).repeat(B, 1).contiguous()
        counts = torch.full((B,), gh * gw, dtype=torch.int32, device=self.device)
        hw = torch.tensor([gh, gw], dtype=torch.int32, device=self.device).repeat(B, 1).contiguous()
        return RaggedGeometry(sel, counts, hw, gh * gw, gh, gw, (B, 3, gh * self.cfg["patch_size"], gw * self.cfg["patch_size"]))

    def bind_pair(self, text_ids: torch.Tensor, text_mask: torch.Tensor, image0, image1, tag: str = "nlvr2") -> PassBuffers:
        """The NLVR2 pair pass (DESIGN.md "NLVR2 fine-tuning"): ONE batch of 2B sequences, sample 2b = (text b, image_0[b]) with token
        type 1 and sample 2b + 1 = (text b, image_1[b]) with token type 2 (rmcl_dims.img_type = -1).  The pooled cls [2B, D] of that pass
        is then, as a view, the [B, 2D] concatenation nlvr2_classifier reads (objectives.py:1006-1010).  The patch geometry is drawn per
        image key in the reference's order (all of image_0, then all of image_1: its two infer calls) and then interleaved."""
        img0 = image0.to(self.device, torch.float32)
        img1 = image1.to(self.device, torch.float32)
        if img0.shape[0] != img1.shape[0]:
            raise ValueError(f"image_0 / image_1 must hold the same number of pairs ({img0.shape[0]} vs {img1.shape[0]})")
        B = img0.shape[0]
        Hm, Wm = max(img0.shape[2], img1.shape[2]), max(img0.shape[3], img1.shape[3])
        img0, img1 = self._pad_to(img0, Hm, Wm).contiguous(), self._pad_to(img1, Hm, Wm).contiguous()
        g0 = self.patch_geometry(img0)
        g1 = self.patch_geometry(img1)
        ps = self.cfg["patch_size"]
        geom = None
        if g0 is not None or g1 is not None:
            gh, gw = Hm // ps, Wm // ps
            g0 = g0 if g0 is not None else self._full_geometry(B, gh, gw)
            g1 = g1 if g1 is not None else self._full_geometry(B, gh, gw)
            il = lambda a, b: torch.stack([a, b], dim=1).reshape((2 * B,) + tuple(a.shape[1:])).contiguous()
            geom = RaggedGeometry(il(g0.sel, g1.sel), il(g0.counts, g1.counts), il(g0.hw, g1.hw), max(g0.n, g1.n), gh, gw,
                                  (2 * B, 3, Hm, Wm))
        img = torch.stack([img0, img1], dim=1).reshape(2 * B, 3, Hm, Wm)
        pb = self._bind(text_ids.to(self.device, torch.int64).repeat_interleave(2, dim=0),
                        text_mask.to(self.device, torch.int64).repeat_interleave(2, dim=0), geom, 2 * B, tag, img_type=-1)
        self._im2patch(img, pb.patches32, geom, 2 * B, Hm, Wm)
        pb.keep_alive = (img,)
        return pb

    def _h2d(self, t: torch.Tensor) -> torch.Tensor:
        """host -> device copy that is asynchronous only out of PINNED memory (a DataLoader with pin_memory): an asynchronous copy out of
        pageable memory leaves it to the runtime when the source is read - blocking there costs microseconds and removes the question"""
        return t.to(self.device, non_blocking=bool(t.device.type == "cpu" and t.is_pinned()))

    def resize_raw(self, raw):
        """``RawUint8Batch`` (decoded bytes at their original sizes) -> ``Uint8Batch`` on the device: MinMaxResize with PIL's integer
        arithmetic in two kernel passes (include/rmcl.h rmcl_image_resize_u8); the tables come from the host (cached per size pair).
        A batch that carries RandAugment plans (``raw.aug``, transform key "decode_uint8_randaug") is augmented first, at its original
        size, by rmcl_randaug_u8."""
        from .vilt.datasets.base_dataset import Uint8Batch
        tgt, hb, hk, vb, vk = raw.tables()
        src = self._h2d(raw.data).contiguous()
        B, Hs, Ws, _ = src.shape
        Hd, Wd = vb.shape[1], hb.shape[1]                               # (the batch extent the tables were packed for)
        # the tables are freshly built pageable host arrays that die with this call: BLOCKING copies (an asynchronous copy out of
        # pageable memory may still be reading it after the arrays are gone); the image bytes themselves belong to the caller's batch
        dev = lambda t: t.to(self.device, non_blocking=False)
        ssz, dsz, hb_d, hk_d, vb_d, vk_d = dev(raw.sizes.contiguous()), dev(tgt.contiguous()), dev(hb), dev(hk), dev(vb), dev(vk)
        aug_alive = ()
        if getattr(raw, "aug", None) is not None:
            # RandAugment first, at the original size (the reference inserts it in front of MinMaxResize): rmcl_randaug_u8 with PIL's bytes.
            # The plan stays on the host - the library checks the op codes there and copies it to the device on the stream
            ops, params = raw.aug
            n_ops = ops.shape[1]
            a_tmp, a_dst = torch.empty_like(src), torch.empty_like(src)
            scratch = torch.empty(int(lib.rmcl_randaug_scratch_bytes(B, n_ops)), dtype=torch.uint8, device=self.device)
            check(lib.rmcl_randaug_u8(P(src), P(ssz), B, Hs, Ws, P(ops), P(params), n_ops, P(a_tmp), P(scratch), P(a_dst), stream_ptr()), "randaug_u8")
            aug_alive, src = (src, ops, params, a_tmp, scratch), a_dst
        tmp = torch.empty(B, Hs, Wd, 3, dtype=torch.uint8, device=self.device)
        dst = torch.empty(B, Hd, Wd, 3, dtype=torch.uint8, device=self.device)
        check(lib.rmcl_image_resize_u8(P(src), P(ssz), B, Hs, Ws, P(dsz), Hd, Wd, P(hb_d), P(hk_d), hk.shape[2], P(vb_d), P(vk_d), vk.shape[2],
                                       P(tmp), P(dst), stream_ptr()), "image_resize_u8")
        out = Uint8Batch(dst, tgt)
        out.keep_alive = (raw.data, src, ssz, dsz, hb_d, hk_d, vb_d, vk_d, tmp) + aug_alive   # until the stream has consumed them
        return out

    def u8_on_device(self, image):
        """``Uint8Batch`` / ``RawUint8Batch`` -> the ``Uint8Batch`` whose bytes lie on the device, its ``sizes`` validated on the host (the
        byte kernels address the batch from them); a raw batch is resized first (``resize_raw``).  A batch that is already there comes
        back as it is, so ``bind_batch`` and ``mpp_bind`` of one pass share ONE copy of the bytes."""
        from .vilt.datasets.base_dataset import Uint8Batch
        if hasattr(image, "tables"):
            image = self.resize_raw(image)
        data, _ = self._u8_ingest(image)
        if data is image.data:
            return image
        out = Uint8Batch(data, image.sizes)
        out.keep_alive = (image, getattr(image, "keep_alive", None))
        return out

    def _u8_ingest(self, u8):
        """the bytes of a Uint8Batch on the device and its sizes [B, 2] on the host, checked against the padded batch"""
        ps = self.cfg["patch_size"]
        data = self._h2d(u8.data).contiguous()
        B, Hh, Ww, _ = data.shape
        sz = torch.as_tensor(u8.sizes)
        if sz.dim() != 2 or tuple(sz.shape) != (B, 2):
            raise ValueError(f"Uint8Batch.sizes must be [B, 2] = (height, width) per sample (got {tuple(sz.shape)} for a batch of {B})")
        if ps != 32 or Hh % ps or Ww % ps or bool((sz % ps != 0).any()):
            raise ValueError(f"uint8 batches need sides that are multiples of the 32-pixel patch (got {tuple(data.shape)}, sizes {sz.tolist()})")
        if bool((sz[:, 0] < 1).any()) or bool((sz[:, 0] > Hh).any()) or bool((sz[:, 1] < 1).any()) or bool((sz[:, 1] > Ww).any()):
            # the ingest kernel addresses img + ((b * Hmax + y) * Wmax + x) * 3 from these extents: an extent outside the padded
            # batch (a hand-built batch, swapped (w, h)) would read past the sample
            raise ValueError(f"Uint8Batch.sizes must satisfy 1 <= h <= {Hh}, 1 <= w <= {Ww} (got {sz.tolist()})")
        if (Hh // ps) * (Ww // ps) > 1024:
            raise ValueError(f"at most 1024 patches per image ({Hh // ps}x{Ww // ps} given)")
        if self._lut is None:
            from .vilt.transforms import normalize_lut
            self._lut = normalize_lut().to(self.device)
        return data, sz.to(torch.int32).cpu()

    def _u8_geometry(self, sz: torch.Tensor, Hh: int, Ww: int, select, max_image_len=None, check_tokens: bool = True):
        """``patch_geometry`` of a byte batch, from its known extents `sz` (host): no selection launch, no read of the counts"""
        from .vilt.datasets.base_dataset import select_from_sizes
        ps, S = self.cfg["patch_size"], self.cfg["image_size"]
        if Hh == S and Ww == S and select is None and bool((sz == S).all()):
            return None
        gh, gw = Hh // ps, Ww // ps
        sel, counts, hw = select_from_sizes(sz, gh, gw, ps)
        sel, counts, n = self._cap_selection(sel, counts, counts, select, max_image_len, check_tokens)   # on the host; to the device only afterwards
        return RaggedGeometry(sel.to(self.device), counts.to(self.device), hw.to(self.device), n, gh, gw, (sz.shape[0], 3, Hh, Ww))

    def _u8_patches(self, data: torch.Tensor, sizes: torch.Tensor, geom, pat: torch.Tensor):
        """bytes [B, Hh, Ww, 3] and sizes [B, 2], both on the device -> the normalised patch rows `pat` (whole grid, or geom's selection)"""
        B, Hh, Ww, _ = data.shape
        ps = self.cfg["patch_size"]
        check(lib.rmcl_image_u8_to_patches(P(data), P(sizes), P(geom.sel) if geom else None, P(geom.counts) if geom else None,
                                           geom.sel.shape[1] if geom else 0, B, geom.n if geom else (Hh // ps) * (Ww // ps), Hh, Ww, ps, P(self._lut),
                                           P(pat), stream_ptr()), "image_u8_to_patches")

    def _bind_uint8(self, text_ids, text_mask, u8, tag, select) -> PassBuffers:
        data, sz = self._u8_ingest(u8)
        B, Hh, Ww, _ = data.shape
        geom = self._u8_geometry(sz, Hh, Ww, select)
        pb = self._bind(text_ids, text_mask, geom, B, tag)
        sizes = self._h2d(u8.sizes)
        self._u8_patches(data, sizes, geom, pb.patches32)
        pb.keep_alive = (data, sizes, u8, getattr(u8, "keep_alive", None))      # until the stream has consumed them
        return pb

    def bind_text(self, like: PassBuffers, text_ids: torch.Tensor, text_mask: torch.Tensor, tag: str) -> PassBuffers:
        """Buffers of another objective/view for the same images (`like.patches32` is shared) with other text."""
        pv = self.twin(like, tag)
        pv.text_ids = text_ids.to(self.device, torch.int64).contiguous()
        pv.text_mask = text_mask.to(self.device, torch.int64).contiguous()
        pv.patches32 = like.patches32
        return pv

    def patches_to_image(self, pat: torch.Tensor, pb: PassBuffers) -> torch.Tensor:
        """patch rows (delta, gradients) of `pb`'s batch back to image layout [B,3,H,W] (zero outside the selected patches)."""
        S = self.cfg["image_size"]
        shape = (pb.B, 3, S, S) if pb.geom is None else tuple(pb.geom.shape)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._im2patch(out, pat, pb.geom, pb.B, shape[2], shape[3], inverse=True)
        return out

    def make_operand(self, pb: PassBuffers, d1=None, d2=None, out=None) -> torch.Tensor:
        """out = cast(patches32 + d1 + d2): the `img_init + img_delta` of pgd_attack_vilt.py:144."""
        out = pb.patchesT if out is None else out
        check(lib.rmcl_add_cast_f32(P(pb.patches32), P(d1), P(d2), P(out), pb.dtype,
                                    I64(pb.patches32.numel()), stream_ptr()), "add_cast")
        return out

    # ---- encoder passes ------------------------------------------------------------------------
    def stream_bit(self, d) -> int:
        """RMCL_MODE_STREAM_ATTN for a pass of more than 256 tokens on an engine built with long_sequences, else 0."""
        return L.MODE_STREAM_ATTN if (self.long_sequences and d.L + 1 + d.P > 256) else 0

    def encoder_forward(self, pb: PassBuffers, key: bool, mode: int, patchesT: torch.Tensor, cls_tail: bool = False,
                        replaced: torch.Tensor = None):
        """replaced [B, P] int32 (MPP): the pass of rmcl_encoder_forward_mpp - the mask token takes the place of those patch embeddings.
        cls_tail: the caller reads only the cls row of every sample of pb.xn (the contrastive objectives: pooler -> head); the
        last block then runs its row-wise part on B rows (include/rmcl.h RMCL_MODE_CLS_TAIL).  Remembered per (buffers, mode):
        the matching encoder_backward picks the compact form by itself.  Under dropout the compact rows draw the masks of the dense
        rows they stand for (csrc/gemm.h drop_row_mul): the tail gives the dense block's numbers there too."""
        if self.lp_stale:
            self.refresh_shadows()
        tail = bool(cls_tail) and pb.B <= 1024 and os.environ.get("RMCL_NO_CLS_TAIL", "0") != "1"
        pb.tail[mode] = tail
        # dropout (reference: live in every train-mode forward incl. the key encoder and the PGD copies, SURVEY
        # quirk 6): a fresh seed per pass, remembered per stash so the matching backward regenerates the masks
        self.pass_counter += 1
        seed = (self.seed_base * 2654435761 + self.pass_counter * 40503) & 0xFFFFFFFF
        p = self.drop_p if self.dropout_on else 0.0
        pb.drop[mode] = (seed, p)
        if self.pass_log is not None:                                  # (tests: which pass drew which masks)
            self.pass_log.append({"seed": seed, "p": p, "mode": mode, "key": bool(key), "B": pb.B, "lane": getattr(pb, "lane", None), "tail": tail})
        p32, plp = (self.k32, self.k_lp) if key else (self.q32, self.q_lp)
        stash = {L.MODE_INFER: None, L.MODE_DATA: pb.stash_data, L.MODE_FULL: pb.stash_full}[mode]
        if replaced is not None:
            if key or tail or self.mpp is None:
                raise L.RmclError("encoder_forward(replaced=...): the MPP pass runs on the query arena of a model with the mpp head, without the cls-only tail")
            check(lib.rmcl_encoder_forward_mpp(C.byref(pb.d), mode | self.stream_bit(pb.d), P(p32), P(plp), P(pb.text_ids), P(pb.text_mask), P(patchesT),
                                               P(pb.co_mask), P(stash), P(pb.workspace), P(pb.xn), C.c_uint32(seed), F(p), self._rg(pb),
                                               self.fold_of(key) if (mode != L.MODE_FULL and pb.dtype == L.BF16) else None, P(replaced),
                                               I64(self.mpp.mt), stream_ptr()), "encoder_forward_mpp")
            return
        check(lib.rmcl_encoder_forward(C.byref(pb.d), mode | (L.MODE_CLS_TAIL if tail else 0) | self.stream_bit(pb.d), P(p32), P(plp), P(pb.text_ids), P(pb.text_mask), P(patchesT),
                                       P(pb.co_mask), P(stash), P(pb.workspace), P(pb.xn), C.c_uint32(seed), F(p), self._rg(pb),
                                       self.fold_of(key) if (mode != L.MODE_FULL and pb.dtype == L.BF16) else None, stream_ptr()),
              "encoder_forward")

    def heads_forward(self, pb: PassBuffers, key: bool, want_q: bool = True, wgrad: bool = True):
        """wgrad=False: the matching heads_backward runs with_grads=False (or not at all): the pooler input is not stashed."""
        head = self.k32 if key else self.q32
        hst = pb.hstash_k if key else pb.hstash_q
        out_q = (pb.k if key else pb.q) if want_q else None
        if not key:
            pb.heads_wgrad = bool(wgrad)
        check(lib.rmcl_heads_forward2(C.byref(pb.d), P(self.q32), P(head), P(pb.xn), P(hst), P(pb.cls), P(out_q),
                                      0 if wgrad else L.HEADS_NO_WGRAD, stream_ptr()), "heads_forward")

    @staticmethod
    def zero_scalar(pb: PassBuffers) -> torch.Tensor:
        """A zeroed 1-element fp32 tensor for a kernel that accumulates into it (``pb.loss_sum`` afterwards): the next slot of a
        pre-zeroed ring - every tiny fill launch on the step's critical path costs ~20 us."""
        if pb.loss_i == pb.loss_ring.numel():
            pb.loss_ring.zero_()
            pb.loss_i = 0
        pb.loss_sum = pb.loss_ring[pb.loss_i:pb.loss_i + 1]
        pb.loss_i += 1
        return pb.loss_sum

    def delta_channel_norm(self, pb: PassBuffers, out: torch.Tensor = None) -> torch.Tensor:
        """out (default: the next zeroed scalar of `pb`, i.e. ``pb.loss_sum``) += sum over the pixels of `pb`'s patch-layout delta of
        the L2 norm over the three channels: the numerator of torch.linalg.norm(delta, dim=1).mean() (objectives.py:184)."""
        out = self.zero_scalar(pb) if out is None else out
        check(lib.rmcl_delta_channel_norm(P(pb.delta), P(out), I64(pb.delta.shape[0]), 3, pb.d.patch_k // 3, stream_ptr()), "delta_norm")
        return out

    def infonce(self, pb: PassBuffers, grad_scale: float, want_dq: bool, metrics: bool = True):
        """metrics=False: the caller reads only loss / dq (PGD passes) - the bf16 engine's form then skips the queue-distance sums.
        bf16 passes run the split-bf16 matrix-core form (include/rmcl.h rmcl_infonce_split_bf16), fp32 passes the exact one."""
        self.zero_scalar(pb)
        if pb.dtype == L.BF16 and not self.exact and os.environ.get("RMCL_INFONCE_EXACT", "0") != "1":
            check(lib.rmcl_infonce_split_bf16(P(pb.q), P(pb.k), P(self.queue), pb.B, 128, I64(self.num_negative),
                                              F(self.cfg["temperature"]), F(grad_scale), P(pb.dq if want_dq else None), P(pb.rows),
                                              P(pb.loss_sum), P(pb.nce_ws), 1 if metrics else 0, stream_ptr()), "infonce")
            return
        check(lib.rmcl_infonce_f32(P(pb.q), P(pb.k), P(self.queue), pb.B, 128, I64(self.num_negative),
                                   F(self.cfg["temperature"]), F(grad_scale), P(pb.dq if want_dq else None), P(pb.rows),
                                   P(pb.loss_sum), P(pb.nce_ws), stream_ptr()), "infonce")

    def heads_backward(self, pb: PassBuffers, dq, dcls_extra, with_grads: bool):
        if with_grads and not getattr(pb, "heads_wgrad", True):
            raise L.RmclError("heads_backward(with_grads=True) after heads_forward(wgrad=False): the pooler input was not stashed")
        check(lib.rmcl_heads_backward(C.byref(pb.d), P(self.q32), P(self.q32), P(pb.hstash_q), P(dq), P(dcls_extra),
                                      P(pb.dcls), P(self.g32 if with_grads else None), P(pb.workspace), stream_ptr()),
              "heads_backward")

    def encoder_backward(self, pb: PassBuffers, mode: int, patchesT, dxn, cls_only: bool, dpatches, dtext=None, replaced: torch.Tensor = None):
        stash = pb.stash_data if mode == L.MODE_DATA else pb.stash_full
        seed, p = pb.drop[mode]
        if replaced is not None:                                       # the backward of an encoder_forward(replaced=...) pass (full-row dxn)
            if cls_only or self.mpp is None:
                raise L.RmclError("encoder_backward(replaced=...): the MPP pass takes a full-row gradient on a model with the mpp head")
            check(lib.rmcl_encoder_backward_mpp(C.byref(pb.d), mode | self.stream_bit(pb.d), P(self.q32), P(self.q_lp), P(pb.text_ids), P(patchesT),
                                                P(pb.co_mask), P(stash), P(pb.workspace), P(dxn), P(dpatches), P(dtext),
                                                P(self.g32 if mode == L.MODE_FULL else None), C.c_uint32(seed), F(p), self._rg(pb),
                                                P(self.weights_T() if pb.dtype == L.BF16 else None), P(replaced), I64(self.mpp.mt), stream_ptr()),
                  "encoder_backward_mpp")
            return
        co = (2 if pb.tail.get(mode) else 1) if cls_only else 0
        if pb.tail.get(mode) and not cls_only:
            raise L.RmclError("encoder_backward: the forward of these buffers kept only the cls rows (cls_tail) - a full-row gradient has nowhere to go")
        check(lib.rmcl_encoder_backward(C.byref(pb.d), mode | self.stream_bit(pb.d), P(self.q32), P(self.q_lp), P(pb.text_ids), P(patchesT),
                                        P(pb.co_mask), P(stash), P(pb.workspace), P(dxn), co, P(dpatches), P(dtext),
                                        P(self.g32 if mode == L.MODE_FULL else None), C.c_uint32(seed), F(p), self._rg(pb),
                                        P(self.weights_T() if pb.dtype == L.BF16 else None), stream_ptr()), "encoder_backward")

    # ---- Barlow-Twins head (include/rmcl.h rmcl_bt_*) --------------------------------------------------------------
    def _head_buffers(self, cls, B: int, tag: str):
        """the per-(batch size, tag) buffers of a head, allocated on first use: cls = BtBuffers / VqaBuffers / Nlvr2Buffers / MlmBuffers"""
        key = (cls, B, tag)
        if key not in self._head_bufs:
            self._head_bufs[key] = cls(self, B)
        return self._head_bufs[key]

    def bt_bufs(self, B: int, tag: str) -> BtBuffers:
        return self._head_buffers(BtBuffers, B, tag)

    def bt_forward(self, bb: BtBuffers, cls: torch.Tensor, training: bool, track: bool):
        """z = barlowtwins_head(cls_feats).  training: batch statistics; track: also update the module's running estimates (the
        module's own head does, the PGD / text attack's deep copy of it does not: pgd_attack_vilt.py:189)."""
        run = self.bt_running if (track or not training) else None
        check(lib.rmcl_bt_head_forward(C.byref(self.bt), P(self.q32), P(cls), bb.B, int(training), P(run), F(0.1), P(bb.stash), P(bb.z),
                                       stream_ptr()), "bt_head_forward")
        if training and track:
            self.bt_tracked += 1
        return bb.z

    def bt_backward(self, bb: BtBuffers, dz: torch.Tensor, training: bool, with_grads: bool):
        check(lib.rmcl_bt_head_backward(C.byref(self.bt), P(self.q32), P(bb.stash), P(dz), bb.B, int(training),
                                        P(self.g32 if with_grads else None), P(bb.dcls), stream_ptr()), "bt_head_backward")
        return bb.dcls

    def bt_loss(self, bb: BtBuffers, zk: torch.Tensor, denom: float, lam: float, grad_scale: float, want_dz: bool, reduce_c=None):
        """loss2 = (on_diag, off_diag) of c = z^T zk / denom (objectives.py:478-484); dz = d(grad_scale (on + lam off))/dz.
        reduce_c: callable run on the correlation matrix between its computation and the loss (the all-reduce of :480)."""
        self.bt_loss_of(bb.z, zk, bb.B, denom, lam, grad_scale, bb.loss2, reduce_c)
        if want_dz:
            check(lib.rmcl_bt_dz(P(zk), P(self.bt_corr), bb.B, self.bt.H3, F(1.0 / denom), P(bb.dz), stream_ptr()), "bt_dz")
        return bb.loss2

    def bt_loss_of(self, z: torch.Tensor, zk: torch.Tensor, B: int, denom: float, lam: float, grad_scale: float, loss2: torch.Tensor,
                   reduce_c=None):
        """(on_diag, off_diag) of c = z^T zk / denom into `loss2` (any 2-float device view); leaves the gradient matrix in
        self.bt_corr."""
        N = self.bt.H3
        check(lib.rmcl_bt_corr(P(z), P(zk), B, N, F(1.0 / denom), P(self.bt_corr), stream_ptr()), "bt_corr")
        if reduce_c is not None:
            reduce_c(self.bt_corr)
        check(lib.rmcl_bt_loss(P(self.bt_corr), N, F(lam), F(grad_scale), P(self.bt_ws), P(loss2), stream_ptr()), "bt_loss")

    def bt_pair_metrics(self, bb: BtBuffers, zk: torch.Tensor):
        check(lib.rmcl_bt_pair_metrics(P(bb.z), P(zk), bb.B, self.bt.H3, P(bb.rows), stream_ptr()), "bt_pair_metrics")
        return bb.rows

    # ---- VQA head (include/rmcl.h rmcl_vqa_*) ------------------------------------------------------------------------
    def vqa_bufs(self, B: int, tag: str) -> VqaBuffers:
        return self._head_buffers(VqaBuffers, B, tag)

    def vqa_targets(self, vb: VqaBuffers, labels, scores):
        """Packs the per-sample label / score lists (``batch["vqa_labels"]`` / ``["vqa_scores"]``, rows may be empty) into ONE pinned
        host buffer [2, B, A] (int32 labels padded with -1, then the fp32 scores' bits) and sends it with one asynchronous copy.
        A label outside [0, vqav2_label_size) is a ValueError (an IndexError in the reference's dense fill, objectives.py:875-877)."""
        B, N = vb.B, self.vqa.N
        if len(labels) != B or len(scores) != B:
            raise ValueError(f"vqa_labels / vqa_scores must have one entry per sample ({len(labels)} / {len(scores)} for a batch of {B})")
        rows_l = [[int(x) for x in (l.tolist() if torch.is_tensor(l) else l)] for l in labels]
        rows_s = [[float(x) for x in (s.tolist() if torch.is_tensor(s) else s)] for s in scores]
        A = max([1] + [len(r) for r in rows_l])
        for b, (rl, rs) in enumerate(zip(rows_l, rows_s)):
            if len(rl) != len(rs):
                raise ValueError(f"sample {b}: {len(rl)} vqa_labels but {len(rs)} vqa_scores")
            bad = [x for x in rl if x < 0 or x >= N]
            if bad:
                raise ValueError(f"sample {b}: vqa label(s) {bad} outside [0, {N}) (vqav2_label_size)")
        if vb._host is None or vb._host.numel() < 2 * B * A:
            vb._host = torch.empty(2 * B * A, dtype=torch.int32, pin_memory=True)
            vb.tab = torch.empty(2 * B * A, dtype=torch.int32, device=self.device)
            vb._copied = None
        self._vqa_host_free(vb)
        host = vb._host[: 2 * B * A].view(2, B, A)
        host[0].fill_(-1)
        host[1].zero_()
        sco = host[1].view(torch.float32)
        for b, (rl, rs) in enumerate(zip(rows_l, rows_s)):
            if rl:
                host[0, b, : len(rl)] = torch.tensor(rl, dtype=torch.int32)
                sco[b, : len(rs)] = torch.tensor(rs, dtype=torch.float32)
        dev = vb.tab[: 2 * B * A].view(2, B, A)
        dev.copy_(host, non_blocking=True)
        vb._copied = torch.cuda.Event()
        vb._copied.record()
        vb.A = A
        vb.labels, vb.scores = dev[0], dev[1].view(torch.float32)
        return vb

    @staticmethod
    def _vqa_host_free(vb: VqaBuffers):
        """the pinned table is rewritten only after the previous batch's copy out of it has completed"""
        ev = getattr(vb, "_copied", None)
        if ev is not None:
            ev.synchronize()

    def vqa_forward(self, vb: VqaBuffers, cls: torch.Tensor):
        check(lib.rmcl_vqa_head_forward(C.byref(self.vqa), P(self.q32), P(cls), vb.B, P(vb.stash), P(vb.logits_p), stream_ptr()),
              "vqa_head_forward")
        return vb.logits

    def vqa_bce(self, vb: VqaBuffers, grad_scale: float, want_dz: bool, scale_dev: torch.Tensor = None, loss2: torch.Tensor = None):
        """loss2 = (vqa_loss, VQAScore) of the batch; rows / argmax per sample; dz (want_dz) = grad_scale [* scale_dev, a device scalar]
        d vqa_loss / d logits."""
        loss2 = vb.loss2 if loss2 is None else loss2
        check(lib.rmcl_vqa_bce(P(vb.logits_p), self.vqa.ldl, P(vb.labels), P(vb.scores), vb.A, vb.B, self.vqa.N, F(grad_scale), P(scale_dev),
                               P(vb.dz if want_dz else None), P(vb.rows), P(vb.argmax), P(loss2), stream_ptr()), "vqa_bce")
        return loss2

    def vqa_backward(self, vb: VqaBuffers, dz: torch.Tensor, with_grads: bool):
        check(lib.rmcl_vqa_head_backward(C.byref(self.vqa), P(self.q32), P(vb.stash), P(dz), vb.B, P(self.g32 if with_grads else None),
                                         P(vb.dcls), stream_ptr()), "vqa_head_backward")
        return vb.dcls

    def vqa_targets_dense(self, vb: VqaBuffers) -> torch.Tensor:
        out = torch.empty(vb.B, self.vqa.N, dtype=torch.float32, device=self.device)
        check(lib.rmcl_vqa_targets_dense(P(vb.labels), P(vb.scores), vb.A, vb.B, self.vqa.N, P(out), self.vqa.N, stream_ptr()),
              "vqa_targets_dense")
        return out

    # ---- NLVR2 head (the VQA head kernels on the nlvr2_classifier struct) + hard-label CE (include/rmcl.h rmcl_nlvr2_ce) ----------
    def nlvr2_bufs(self, B: int, tag: str) -> Nlvr2Buffers:
        return self._head_buffers(Nlvr2Buffers, B, tag)

    def nlvr2_labels(self, nb: Nlvr2Buffers, answers):
        """batch["answers"] (bools, or 0 / 1; objectives.py:1012-1013 casts them to long) -> nb.labels.  Anything else is a ValueError
        (the reference's cross_entropy raises on a target outside [0, 2))."""
        vals = answers.tolist() if torch.is_tensor(answers) else list(answers)
        if len(vals) != nb.B:
            raise ValueError(f"answers must have one entry per pair ({len(vals)} for {nb.B} pairs)")
        ints = [int(v) for v in vals]
        if any(v not in (0, 1) for v in ints):
            raise ValueError(f"NLVR2 answers must be True / False (got {vals})")
        nb.labels.copy_(torch.tensor(ints, dtype=torch.int32))
        return nb.labels

    def nlvr2_forward(self, nb: Nlvr2Buffers, cls2: torch.Tensor):
        """logits [B, 2] = nlvr2_classifier(cls2 [B, 2 hidden])."""
        check(lib.rmcl_vqa_head_forward(C.byref(self.nlvr2), P(self.q32), P(cls2), nb.B, P(nb.stash), P(nb.logits_p), stream_ptr()),
              "nlvr2_head_forward")
        return nb.logits

    def nlvr2_ce(self, nb: Nlvr2Buffers, grad_scale: float, want_dz: bool, scale_dev: torch.Tensor = None, ref: "Nlvr2Buffers" = None,
                 stats: torch.Tensor = None):
        """stats = (mean CE, correct rows, rows whose argmax differs from ref's logits); rows / argmax per pair; dz (want_dz) =
        grad_scale [* scale_dev] d CE / d logits."""
        stats = nb.stats if stats is None else stats
        check(lib.rmcl_nlvr2_ce(P(nb.logits_p), self.nlvr2.ldl, P(nb.labels), nb.B, self.nlvr2.N, F(grad_scale), P(scale_dev),
                                P(nb.dz if want_dz else None), P(nb.rows), P(nb.argmax), P(ref.logits_p if ref is not None else None),
                                self.nlvr2.ldl, P(stats), stream_ptr()), "nlvr2_ce")
        return stats

    def nlvr2_backward(self, nb: Nlvr2Buffers, dz: torch.Tensor, with_grads: bool):
        check(lib.rmcl_vqa_head_backward(C.byref(self.nlvr2), P(self.q32), P(nb.stash), P(dz), nb.B, P(self.g32 if with_grads else None),
                                         P(nb.dcls), stream_ptr()), "nlvr2_head_backward")
        return nb.dcls

    # ---- text attack on the fine-tuning tasks (include/rmcl.h rmcl_word_saliency) -------------------------------------------
    def word_saliency(self, g: torch.Tensor, spans: torch.Tensor, L_: int, row0: int = 0, row_step: int = 1, out: torch.Tensor = None):
        """out [B, W] = L1 norm of the mean saliency gradient over each word's sub-word tokens.  g: the fp32 `dtext` buffer of
        encoder_backward, [R * L_, D] (or [R, L_, D]); spans [B, W, 2] int32 on the device (first token position counting [CLS] as 0,
        token count; count 0 = padding entry -> 0); sentence b reads sequence row0 + b * row_step of g."""
        B, W = int(spans.shape[0]), int(spans.shape[1])
        D = int(g.shape[-1])
        R = g.numel() // (L_ * D)
        if g.dtype != torch.float32 or spans.dtype != torch.int32 or not g.is_contiguous() or not spans.is_contiguous() or spans.shape[2] != 2:
            raise L.RmclError("word_saliency: g must be contiguous fp32 and spans contiguous int32 [B, W, 2]")
        if row0 < 0 or row_step < 1 or row0 + (B - 1) * row_step >= R:
            raise L.RmclError(f"word_saliency: sequence {row0} + {B - 1} * {row_step} is outside the {R} sequences of the gradient buffer")
        out = torch.empty(B, W, dtype=torch.float32, device=self.device) if out is None else out
        check(lib.rmcl_word_saliency(P(g), P(spans), P(out), B, W, L_, D, row0, row_step, stream_ptr()), "word_saliency")
        return out

    # ---- row top-k of the prediction API (include/rmcl.h rmcl_rows_topk) -----------------------------------------------------
    TOPK_MODES = {"raw": L.TOPK_RAW, "softmax": L.TOPK_SOFTMAX, "sigmoid": L.TOPK_SIGMOID}

    def rows_topk(self, x: torch.Tensor, k: int, mode: str = "raw", want_lse: bool = False):
        """(idx [R, k] int32, val [R, k], prob [R, k] or None for "raw"[, lse [R] with want_lse]) of a 2-D fp32 device tensor whose last
        dimension is contiguous; the row stride is read from the tensor, so a column slice or a pitched view needs no copy.  Larger
        value first, ties to the smaller column, NaN never selected; slots a row cannot fill hold idx -1, val -inf, prob 0.  No host
        synchronisation.  Shape and argument errors are ValueErrors raised here, before the launch."""
        if mode not in Engine.TOPK_MODES:
            raise ValueError(f"rows_topk: mode must be one of {sorted(Engine.TOPK_MODES)} (got {mode!r})")
        if want_lse and mode != "softmax":
            raise ValueError("rows_topk: want_lse needs mode='softmax' (the log-sum-exp is formed by that mode's launch)")
        if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("rows_topk: x must be a 2-D fp32 tensor")
        if not x.is_cuda:
            raise ValueError("rows_topk: x must be on the device (rmcl_amd has no CPU path)")
        R, Cn = int(x.shape[0]), int(x.shape[1])
        k = int(k)
        if Cn < 1 or k < 1 or k > min(Cn, L.TOPK_MAX):
            raise ValueError(f"rows_topk: k must be in 1 .. min(columns, {L.TOPK_MAX}) (k = {k}, columns = {Cn})")
        if Cn > 1 and x.stride(1) != 1:
            raise ValueError("rows_topk: the last dimension of x must be contiguous (take the top-k of a transposed matrix on a contiguous copy)")
        ld = int(x.stride(0)) if R > 1 else Cn
        if ld < Cn:
            raise ValueError(f"rows_topk: rows of x overlap (row stride {ld} < {Cn} columns)")
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=x.device)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=x.device)
        idx, val = i32(R, k), f32(R, k)
        prob = None if mode == "raw" else f32(R, k)
        lse = f32(R) if want_lse else None
        check(lib.rmcl_rows_topk(P(x), I64(ld), R, Cn, k, Engine.TOPK_MODES[mode], P(idx), P(val), P(prob), P(lse), stream_ptr()), "rows_topk")
        return (idx, val, prob, lse) if want_lse else (idx, val, prob)

    # ---- word-patch alignment maps of the prediction API (include/rmcl.h rmcl_ipot_plan_f32, rmcl_align_heat) -----------------
    def ipot_plan(self, cost: torch.Tensor, txt_valid: torch.Tensor, img_valid: torch.Tensor, beta: float, iters: int) -> torch.Tensor:
        """The transport plan T [B, Li, Lt] of ``ipot(cost, ..., beta, iters, k = 1)``: cost [B, Lt, ld >= Li] fp32 as
        rmcl_wpa_cost_finish leaves it, txt_valid [B, Lt] / img_valid [B, Li] int32, all contiguous on the device.  Limit errors are
        ValueErrors raised here, before the launch."""
        if not (torch.is_tensor(cost) and cost.dim() == 3 and cost.dtype == torch.float32 and cost.is_cuda and cost.is_contiguous()):
            raise ValueError("ipot_plan: cost must be a contiguous fp32 device tensor [B, Lt, ld]")
        B, Lt, ld = (int(v) for v in cost.shape)
        for name, t in (("txt_valid", txt_valid), ("img_valid", img_valid)):
            if not (torch.is_tensor(t) and t.dim() == 2 and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.shape[0] == B):
                raise ValueError(f"ipot_plan: {name} must be a contiguous int32 device tensor [B = {B}, ...]")
        Li, iters, beta = int(img_valid.shape[1]), int(iters), float(beta)
        if txt_valid.shape[1] != Lt or not 1 <= Lt <= L.IPOT_PLAN_MAX_LT:
            raise ValueError(f"ipot_plan: the text length must be in 1 .. {L.IPOT_PLAN_MAX_LT} and that of txt_valid (cost has {Lt}, txt_valid {txt_valid.shape[1]})")
        if not 1 <= Li <= min(ld, L.IPOT_PLAN_MAX_LI):
            raise ValueError(f"ipot_plan: the image length must be in 1 .. {L.IPOT_PLAN_MAX_LI} and at most the pitch of cost (got {Li}, pitch {ld})")
        if not 1 <= iters <= L.IPOT_PLAN_MAX_ITERS:
            raise ValueError(f"ipot_plan: iterations must be in 1 .. {L.IPOT_PLAN_MAX_ITERS} (got {iters})")
        if not beta > 0.0:
            raise ValueError(f"ipot_plan: beta must be > 0 (got {beta})")
        T = torch.empty(B, Li, Lt, dtype=torch.float32, device=cost.device)
        check(lib.rmcl_ipot_plan_f32(P(cost), P(txt_valid), P(img_valid), P(T), B, Lt, Li, ld, F(beta), iters, stream_ptr()), "ipot_plan")
        return T

    @staticmethod
    def nearest_table(src: int, dst: int) -> List[int]:
        """source index of every output pixel of PIL's NEAREST resize of `src` pixels to `dst`: the centre 0.5 * src / dst advanced by
        src / dst per pixel IN DOUBLE, accumulated, truncated and cut at src - 1.  (The closed form floor((x + 0.5) * src / dst) differs
        from PIL's accumulation at some sizes.)"""
        step = float(src) / float(dst)
        xo, out = 0.5 * step, []
        for _ in range(dst):
            out.append(min(int(xo), src - 1))
            xo += step
        return out

    def align_heat(self, plan: torch.Tensor, patch_index: torch.Tensor, txt_valid: torch.Tensor, grid_hw, token=None, size=None):
        """(grid, heat [B, Lt, H, W] fp32, flat [B, Lt] int32, alpha [B, Hout, Wout] uint8 or None) of a plan [B, Li, Lt] (include/rmcl.h
        rmcl_align_heat).  patch_index [B, Li - 1] int32: the flat grid cell of every image slot behind the cls slot (negative: none);
        token: None, or one text position per sample (a list of B ints, on the host) whose alpha bytes are wanted at size = (Hout, Wout)."""
        H, W = int(grid_hw[0]), int(grid_hw[1])
        if not (torch.is_tensor(plan) and plan.dim() == 3 and plan.dtype == torch.float32 and plan.is_cuda and plan.is_contiguous()):
            raise ValueError("align_heat: plan must be a contiguous fp32 device tensor [B, Li, Lt]")
        B, Li, Lt = (int(v) for v in plan.shape)
        if H < 1 or W < 1 or H * W > L.ALIGN_MAX_CELLS:
            raise ValueError(f"align_heat: the grid must have 1 .. {L.ALIGN_MAX_CELLS} cells (got {H} x {W})")
        if not (patch_index.dtype == torch.int32 and patch_index.is_cuda and patch_index.is_contiguous() and tuple(patch_index.shape) == (B, Li - 1)):
            raise ValueError(f"align_heat: patch_index must be a contiguous int32 device tensor [{B}, {Li - 1}]")
        if not (txt_valid.dtype == torch.int32 and txt_valid.is_cuda and txt_valid.is_contiguous() and tuple(txt_valid.shape) == (B, Lt)):
            raise ValueError(f"align_heat: txt_valid must be a contiguous int32 device tensor [{B}, {Lt}]")
        dev = plan.device
        grid = torch.empty(B, Lt, H, W, dtype=torch.float32, device=dev)
        heat = torch.empty(B, Lt, H, W, dtype=torch.float32, device=dev)
        flat = torch.empty(B, Lt, dtype=torch.int32, device=dev)
        alpha = tok = tab = None
        Ho = Wo = 0
        if token is not None:
            token = [int(v) for v in token]
            if len(token) != B or any(not 0 <= v < Lt for v in token):
                raise ValueError(f"align_heat: token must hold one text position in 0 .. {Lt - 1} per sample ({B} samples; got {token})")
            Ho, Wo = (int(size[0]), int(size[1])) if size is not None and len(size) == 2 else (0, 0)
            if not (1 <= Ho <= 16384 and 1 <= Wo <= 16384):
                raise ValueError(f"align_heat: size must be (height, width) with both in 1 .. 16384 (got {size})")
            # the position of every sample and the two index tables: one upload
            up = self._h2d(torch.tensor(token + Engine.nearest_table(H, Ho) + Engine.nearest_table(W, Wo), dtype=torch.int32))
            tok, tab = up[:B], up[B:]
            alpha = torch.empty(B, Ho, Wo, dtype=torch.uint8, device=dev)
        check(lib.rmcl_align_heat(P(plan), P(patch_index), P(txt_valid), B, Lt, Li, H, W, P(grid), P(heat), P(flat), P(tok), P(tab), Ho, Wo,
                                  P(alpha), stream_ptr()), "align_heat")
        return grid, heat, flat, alpha

    # ---- MLM head (include/rmcl.h rmcl_mlm_*) ------------------------------------------------------------------------
    def mlm_bufs(self, B: int, tag: str) -> MlmBuffers:
        return self._head_buffers(MlmBuffers, B, tag)

    def mlm_weights_T(self) -> torch.Tensor:
        """decoder.weight^T [D, vocab rounded up to 128] in the engine's operand type, re-derived when the masters changed"""
        if self.lp_stale:
            self.refresh_shadows()
        if self.mlm_wT is None:
            ldv = (self.mlm.V + 127) // 128 * 128
            self.mlm_wT = torch.empty(self.mlm.D, ldv, dtype=torch.bfloat16 if self.dtype == L.BF16 else torch.float32, device=self.device)
        if self.mlm_wt_stale:
            check(lib.rmcl_mlm_weight_transpose(C.byref(self.mlm), P(self.q32), P(self.mlm_wT), self.dtype, stream_ptr()), "mlm_weight_transpose")
            self.mlm_wt_stale = False
        return self.mlm_wT

    def mlm_bind(self, mb: MlmBuffers, labels: torch.Tensor, N: int, all_rows: bool = False) -> MlmBuffers:
        """Validates ``text_labels_mlm`` [B, L] (a label other than -100 outside [0, vocab_size) is a ValueError here, on the host - never
        a device fault) and builds the compaction on the device.  Labels that arrive on the host (a DataLoader's batch) are checked and
        counted there for free, and the count only sizes the launches; labels already on the device cost one read-back of two scalars.
        N: token rows per sample of the xn the rows will be gathered from.  all_rows: list every position (the dense-logits pass)."""
        V = self.mlm.V
        if tuple(labels.shape) != (mb.B, mb.L):
            raise ValueError(f"text_labels_mlm must be [B, max_text_len] = {(mb.B, mb.L)} (got {tuple(labels.shape)})")
        lab = labels.to(torch.int64)
        on = lab != -100
        bad = on & ((lab < 0) | (lab >= V))
        n_bad, n = (int(v) for v in torch.stack([bad.sum(), on.sum()]).tolist())
        if n_bad:
            raise ValueError(f"text_labels_mlm: {n_bad} label(s) outside [0, {V}) (vocab_size) other than the ignore index -100")
        mb.labels = lab.to(self.device).contiguous()
        mb.bind_rows(n, all_rows)
        check(lib.rmcl_mlm_compact(P(mb.labels), mb.M, mb.L, int(N), V, int(all_rows), P(mb.idx), P(mb.lab), P(mb.count), stream_ptr()),
              "mlm_compact")
        return mb

    def _pred_forward(self, fn, what: str, head, hb: CompactedHeadBuffers, xn: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
        """rmcl_mlm_forward / rmcl_mpp_forward (one argument list) on the bound compacted buffers `hb`"""
        if self.lp_stale:
            self.refresh_shadows()
        stats = torch.empty(3, dtype=torch.float32, device=self.device) if stats is None else stats
        check(fn(C.byref(head), P(self.q32), P(self.q_lp), self.dtype, P(xn), P(hb.idx), P(hb.lab), P(hb.count), hb.rows,
                 P(hb.ws), P(hb.lse), P(hb.rowloss), P(hb.argmax), P(stats), stream_ptr()), what)
        return stats

    def _pred_backward(self, fn, what: str, head, hb: CompactedHeadBuffers, grad_scale, scale_dev, dxn, with_grads, *operands):
        """rmcl_mlm_backward / rmcl_mpp_backward; `operands`: what the head passes between the shadow arena and the dtype (MLM: W^T)"""
        check(fn(C.byref(head), P(self.q32), P(self.q_lp), *(P(o) for o in operands), self.dtype, P(hb.idx), P(hb.lab), P(hb.count), hb.rows,
                 P(hb.ws), P(hb.lse), F(grad_scale), P(scale_dev), P(self.g32 if with_grads else None), P(dxn), stream_ptr()), what)

    def mlm_forward(self, mb: MlmBuffers, xn: torch.Tensor, stats: torch.Tensor = None) -> torch.Tensor:
        """stats = (mlm_loss, rows with argmax == label, n) of the bound batch; per compacted row mb.lse / .rowloss / .argmax."""
        return self._pred_forward(lib.rmcl_mlm_forward, "mlm_forward", self.mlm, mb, xn, stats)

    def mlm_backward(self, mb: MlmBuffers, grad_scale: float, scale_dev: torch.Tensor, dxn: torch.Tensor, with_grads: bool = True):
        """CE gradient (recomputed) -> decoder -> transform -> stored into the zero-filled dxn [B N, D]; head gradients into the arena."""
        self._pred_backward(lib.rmcl_mlm_backward, "mlm_backward", self.mlm, mb, grad_scale, scale_dev, dxn, with_grads, self.mlm_weights_T())

    def mlm_logits(self, mb: MlmBuffers, rows_out: int) -> torch.Tensor:
        """dense logits [rows_out, vocab] of the first rows_out compacted rows of the last mlm_forward on `mb`"""
        out = torch.empty(rows_out, self.mlm.V, dtype=torch.float32, device=self.device)
        check(lib.rmcl_mlm_logits(C.byref(self.mlm), P(self.q32), P(self.q_lp), self.dtype, P(mb.ws), mb.rows, rows_out, P(out), I64(self.mlm.V),
                                  stream_ptr()), "mlm_logits")
        return out

    # ---- MPP head (include/rmcl.h rmcl_mpp_*) ------------------------------------------------------------------------
    def mpp_bufs(self, B: int, tag: str, Pn: int) -> MppBuffers:
        key = (MppBuffers, B, tag, Pn)
        if key not in self._head_bufs:
            self._head_bufs[key] = MppBuffers(self, B, Pn)
        return self._head_bufs[key]

    def mpp_bind(self, mp: MppBuffers, img: torch.Tensor, pb: PassBuffers, masked: torch.Tensor, replaced: torch.Tensor,
                 all_rows: bool = False) -> MppBuffers:
        """``mpp_labels_masks``, then ``mpp_compact``: the labels and gathered masks of the batch, and the compaction of its masked valid
        slots.  A pixel mean outside [0, 1] (pixels outside [-1, 1]) is a ValueError (``mpp_check_labels``), like the reference's
        cross_entropy raising on a label outside 0..255."""
        self.mpp_labels_masks(mp, img, pb, masked, replaced)
        return self.mpp_compact(mp, pb, all_rows)

    def mpp_labels_masks(self, mp: MppBuffers, img: torch.Tensor, pb: PassBuffers, masked: torch.Tensor, replaced: torch.Tensor):
        """Labels of the batch's image slots from the float image `img` [B, 3, H, W] (on the device) into mp.labels, and the two full-grid
        masks [B, G] gathered through `pb`'s patch selection into mp.masked / mp.replaced [B, P] (pad slots: 0).  mp.n_masked: the
        host-known number of masked patches (it only sizes the launches; n stays on the device).
        `img` may be a ``Uint8Batch`` / ``RawUint8Batch`` instead: the labels then come from the bytes (rmcl_mpp_labels_u8: the same
        integers as from ``float_image()``, which is never built), G from the batch's ``shape``."""
        u8 = None
        if not torch.is_tensor(img):
            u8 = self.u8_on_device(img)
            u8_sizes = self._h2d(u8.sizes)
            mp.keep_alive = (u8, u8_sizes)                                    # until the stream has consumed them
            img = u8
        B, _, Hh, Ww = img.shape
        ps = int(self.cfg["patch_size"])
        if ps != 32:
            raise NotImplementedError("MPP labels are built for patch_size = 32")
        G = (Hh // ps) * (Ww // ps)
        if tuple(masked.shape) != (B, G) or tuple(replaced.shape) != (B, G):
            raise ValueError(f"mpp masks must be [B, G] = {(B, G)} over the full patch grid (got {tuple(masked.shape)}, {tuple(replaced.shape)})")
        d, geom = pb.d, pb.geom
        Pn = d.P
        n_host = int(masked.sum()) if masked.device.type == "cpu" else B * Pn
        mk = masked.to(self.device).to(torch.int32)
        rp = (replaced.to(self.device) & masked.to(self.device)).to(torch.int32) if replaced.dtype == torch.bool else replaced.to(self.device, torch.int32) * mk
        if u8 is not None:
            check(lib.rmcl_mpp_labels_u8(P(u8.data), P(u8_sizes), B, Hh, Ww, P(self._lut), P(geom.sel) if geom else None,
                                         P(geom.counts) if geom else None, geom.sel.shape[1] if geom else 0, Ww // ps, Pn, P(mp.labels),
                                         stream_ptr()), "mpp_labels_u8")
        elif geom is None:
            check(lib.rmcl_mpp_labels(P(img), B, Hh, Ww, None, None, 0, Ww // ps, Pn, P(mp.labels), stream_ptr()), "mpp_labels")
        else:
            check(lib.rmcl_mpp_labels(P(img), B, Hh, Ww, P(geom.sel), P(geom.counts), geom.sel.shape[1], geom.gw, Pn, P(mp.labels), stream_ptr()),
                  "mpp_labels")
        if geom is None:
            mp.masked, mp.replaced = mk.contiguous(), rp.contiguous()
        else:
            sel = geom.sel[:, :Pn].to(torch.int64).clamp_(0, G - 1)
            valid = (torch.arange(Pn, device=self.device)[None, :] < geom.counts[:, None]).to(torch.int32)
            mp.masked = (torch.gather(mk, 1, sel) * valid).contiguous()
            mp.replaced = (torch.gather(rp, 1, sel) * valid).contiguous()
        mp.n_masked = min(n_host, B * Pn)

    def mpp_compact(self, mp: MppBuffers, pb: PassBuffers, all_rows: bool = False) -> MppBuffers:
        """The compaction of mp.labels / mp.masked for `pb`'s row layout: the masked valid slots, or (all_rows, the dense-logits pass) every
        image row.  The launch extent comes from mp.n_masked."""
        d = pb.d
        mp.bind_rows(mp.n_masked, all_rows)
        check(lib.rmcl_mpp_compact(P(mp.labels), P(mp.masked), mp.B, d.P, d.L, d.L + 1 + d.P, int(all_rows), mp.cap, P(mp.idx), P(mp.lab), P(mp.count),
                                   stream_ptr()), "mpp_compact")
        return mp

    def mpp_check_labels(self, mp: MppBuffers):
        """count[1] of the compaction: label entries outside 0..255 (one read-back of two ints)"""
        n_bad = int(mp.count.tolist()[1])
        if n_bad:
            raise ValueError(f"mpp: {n_bad} patch label(s) outside 0..255 - the pixels of `image` must lie in [-1, 1] (the labels are "
                             "trunc(mean(image * 0.5 + 0.5) * 255) per patch and channel)")

    def mpp_forward(self, mp: MppBuffers, xn: torch.Tensor, stats: torch.Tensor = None) -> torch.Tensor:
        """stats = (mpp_loss, correct (row, channel) pairs, labelled pairs) of the bound batch; per listed row mp.lse / .rowloss / .argmax."""
        return self._pred_forward(lib.rmcl_mpp_forward, "mpp_forward", self.mpp, mp, xn, stats)

    def mpp_backward(self, mp: MppBuffers, grad_scale: float, scale_dev: torch.Tensor, dxn: torch.Tensor, with_grads: bool = True):
        """CE gradient -> decoder -> transform -> stored into the zero-filled dxn [B N, D]; head gradients into the arena."""
        self._pred_backward(lib.rmcl_mpp_backward, "mpp_backward", self.mpp, mp, grad_scale, scale_dev, dxn, with_grads)

    def mpp_logits(self, mp: MppBuffers, rows_out: int) -> torch.Tensor:
        """dense logits [rows_out, 768] of the first rows_out listed rows of the last mpp_forward on `mp`"""
        out = torch.empty(rows_out, 768, dtype=torch.float32, device=self.device)
        check(lib.rmcl_mpp_logits(C.byref(self.mpp), P(mp.ws), mp.rows, rows_out, P(out), stream_ptr()), "mpp_logits")
        return out

    # ---- IRTR: rank head, visual_embed, the cached rank pass (include/rmcl.h "Image-text retrieval") ------------------------------------
    def rank_params(self, arena: torch.Tensor = None):
        """(weight [D], bias [1]) of rank_output = row 1 of the ITM head's slots, in `arena` (default: the parameters)."""
        a = self.q32 if arena is None else arena
        lay, D = self.layout, int(self.cfg["hidden_size"])
        return a[lay.itm_w + D:lay.itm_w + 2 * D], a[lay.itm_b + 1:lay.itm_b + 2]

    def irtr_score(self, cls: torch.Tensor, scores: torch.Tensor, out_index: torch.Tensor = None):
        """scores[out_index[i] or i] = rank_output(cls[i])."""
        w, b = self.rank_params()
        check(lib.rmcl_irtr_score(P(cls), I64(cls.stride(0)), P(w), P(b), cls.shape[0], cls.shape[1], P(scores), P(out_index),
                                  I64(scores.numel()), stream_ptr()), "irtr_score")
        return scores

    def irtr_ce(self, scores: torch.Tensor, B: int, R: int, grad_scale: float, dscore=None, scale_dev=None, rows=None, stats=None):
        stats = torch.empty(2, dtype=torch.float32, device=self.device) if stats is None else stats
        check(lib.rmcl_irtr_ce(P(scores), B, R, F(grad_scale), P(scale_dev), P(dscore), P(rows), P(stats), stream_ptr()), "irtr_ce")
        return stats

    def irtr_backward(self, dscore: torch.Tensor, cls: torch.Tensor, dcls: torch.Tensor, with_grads: bool):
        w, _ = self.rank_params()
        gw, gb = self.rank_params(self.g32) if with_grads else (None, None)
        check(lib.rmcl_irtr_bwd(P(dscore), P(cls), I64(cls.stride(0)), P(w), cls.shape[0], cls.shape[1], P(dcls), P(gw), P(gb), stream_ptr()),
              "irtr_bwd")
        return dcls

    def token_limit_error(self, n_patches: int):
        """the message of a rank pass / recall evaluation that cannot run: names the ways out"""
        Lt = int(self.cfg["max_text_len"])
        if self.long_sequences:
            return NotImplementedError(
                f"{n_patches} image patches + 1 cls + {Lt} text tokens = {n_patches + 1 + Lt} tokens exceed the 512-token limit of the streaming "
                f"bf16 attention kernels (long_sequences): set max_image_len <= {511 - Lt}, or build the model with compute_dtype='f32' (the "
                f"fp32 engine has no such limit)")
        return NotImplementedError(
            f"{n_patches} image patches + 1 cls + {Lt} text tokens = {n_patches + 1 + Lt} tokens exceed the 256-token limit of the fused bf16 "
            f"attention kernels: set max_image_len <= {255 - Lt}, or build the model with compute_dtype='f32' (the fp32 engine has no such limit), "
            f"or set config['long_sequences'] = True (streaming attention kernels, up to 512 tokens)")

    def patch_count(self, images: torch.Tensor, max_image_len=None) -> int:
        """the padded image length n that visual_embed(images, max_image_len) would produce, without embedding or drawing anything
        (patch_geometry's count and cap, not its selection: the host generator is left alone)"""
        img = images.to(self.device, torch.float32).contiguous()
        B, Cc, Hh, Ww = img.shape
        ps = self.cfg["patch_size"]
        if Cc != 3 or Hh % ps or Ww % ps or (Hh // ps) * (Ww // ps) > 1024:
            return self.patch_geometry(img, None, max_image_len=max_image_len, check_tokens=False).n      # raises its ValueError
        sel = torch.empty(B, (Hh // ps) * (Ww // ps), dtype=torch.int32, device=self.device)
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        hw = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        check(lib.rmcl_patch_select(P(img), B, 3, Hh, Ww, ps, P(sel), P(counts), P(hw), stream_ptr()), "patch_select")
        n = int(counts.max())
        mil = self.cfg.get("max_image_len", -1) if max_image_len is None else max_image_len
        return min(n, mil) if isinstance(mil, int) and mil > 0 else n

    def visual_embed(self, images: torch.Tensor, max_image_len=None, select: torch.Tensor = None, mpp_masks=None):
        """VisionTransformer.visual_embed (vision_transformer.py:559-677, mask_it=False): (embeds [B, 1 + n, D] f32 WITHOUT the token-type
        row, masks [B, 1 + n] int64, patch_index [B, n, 2]).  The 256-token limit does not apply here (the pass has no text): the rank pass
        checks; with long_sequences an image that cannot fit 512 tokens with its text is refused here already.
        Runs once per image, so its buffers are allocated per call (the caching allocator hands the same blocks back)."""
        if self.lp_stale:
            self.refresh_shadows()
        ps = self.cfg["patch_size"]
        u8 = None
        if torch.is_tensor(images):
            img = images.to(self.device, torch.float32).contiguous()
            B, _, Hh, Ww = img.shape
            geom = self.patch_geometry(img, select, max_image_len=max_image_len, check_tokens=False)
        else:                                                          # Uint8Batch / RawUint8Batch: geometry from the extents, rows from the bytes
            img = u8 = self.u8_on_device(images)
            B, _, Hh, Ww = u8.shape
            geom = self._u8_geometry(self._u8_ingest(u8)[1], Hh, Ww, select, max_image_len=max_image_len, check_tokens=False)
        g = self.cfg["image_size"] // ps
        n = g * g if geom is None else geom.n
        if self.long_sequences and n + 1 + int(self.cfg["max_text_len"]) > self.token_cap:
            # 512 tokens is also where the library's own dims check ends: name the ways out instead.  compute_irtr_recall never gets here:
            # it takes patch_count() first and raises on every rank together
            raise self.token_limit_error(n)
        d = self.dims(B, None, n)
        ws = torch.empty(int(lib.rmcl_workspace_bytes(C.byref(d))), dtype=torch.uint8, device=self.device)
        pat32 = torch.empty(B * n, d.patch_k, dtype=torch.float32, device=self.device)
        op = pat32 if self.dtype == L.F32 else torch.empty(B * n, d.patch_k, dtype=torch.bfloat16, device=self.device)
        rg = None
        if u8 is None:
            self._im2patch(img, pat32, geom, B, Hh, Ww)
        else:
            self._u8_patches(u8.data, self._h2d(u8.sizes), geom, pat32)
        if geom is None:
            ii, jj = torch.meshgrid(torch.arange(g), torch.arange(g), indexing="ij")
            patch_index = torch.stack([ii, jj], dim=-1).reshape(1, g * g, 2).expand(B, -1, -1)
        else:
            pos_tok = torch.empty(B, n + 1, d.D, dtype=torch.float32, device=self.device)
            rg = L.Ragged(sel=geom.sel.data_ptr(), counts=geom.counts.data_ptr(), hw=geom.hw.data_ptr(), sel_ld=geom.sel.shape[1],
                          gw=geom.gw, G0=g, pos_tok=pos_tok.data_ptr(), dpos_tok=0)
            sel = geom.sel[:, :n].to(torch.int64)
            patch_index = torch.stack([sel // geom.gw, sel % geom.gw], dim=-1)
        if self.dtype != L.F32:
            check(lib.rmcl_add_cast_f32(P(pat32), None, None, P(op), self.dtype, I64(pat32.numel()), stream_ptr()), "add_cast")
        out = torch.empty(B, n + 1, d.D, dtype=torch.float32, device=self.device)
        masks = torch.empty(B, n + 1, dtype=torch.int32, device=self.device)
        if mpp_masks is not None:
            # visual_embed(mask_it=True): the full-grid masks (masked, replaced) [B, G] go through mpp_bind like compute_mpp's - labels of
            # this call's slots, masks gathered through its selection - and the MppBuffers come back as the fourth value
            import types
            mp = self.mpp_bind(self.mpp_bufs(B, "visual_embed", n), img, types.SimpleNamespace(d=d, geom=geom), mpp_masks[0], mpp_masks[1])
            check(lib.rmcl_visual_embed_mpp(C.byref(d), P(self.q32), P(self.q_lp), P(op), C.byref(rg) if rg is not None else None, P(ws), P(out),
                                            P(masks), P(mp.replaced), I64(self.mpp.mt), stream_ptr()), "visual_embed_mpp")
            return out, masks.to(torch.int64), patch_index, mp
        check(lib.rmcl_visual_embed(C.byref(d), P(self.q32), P(self.q_lp), P(op), C.byref(rg) if rg is not None else None, P(ws), P(out),
                                    P(masks), stream_ptr()), "visual_embed")
        return out, masks.to(torch.int64), patch_index

    def rank_forward(self, text_ids: torch.Tensor, text_mask: torch.Tensor, embeds: torch.Tensor, masks: torch.Tensor, img_of: torch.Tensor,
                     n_patches: int, cls_tail: bool = True) -> RankPass:
        """One encoder pass over the sequences (text b, cached image img_of[b]) and the pooler: embeds [n_img, ld_tok, D] f32 / masks
        [n_img, ld_tok] int32 are the cache of visual_embed outputs, n_patches <= ld_tok - 1 the padded image length of THIS pass.
        Returns the pass buffers (.cls [B, D] pooled, .xn, .co_mask)."""
        if self.lp_stale:
            self.refresh_shadows()
        B = int(text_ids.shape[0])
        if embeds.dtype != torch.float32 or masks.dtype != torch.int32 or img_of.dtype != torch.int32 or not (
                embeds.is_contiguous() and masks.is_contiguous() and img_of.is_contiguous()):
            raise ValueError("rank_forward: embeds f32 [n_img, ld_tok, D], masks / img_of int32, all contiguous")
        n_img, ld_tok, D = embeds.shape
        if tuple(masks.shape) != (n_img, ld_tok) or img_of.numel() != B or n_patches + 1 > ld_tok or n_patches < 1 or D != self.cfg["hidden_size"]:
            raise ValueError(f"rank_forward: shapes do not fit (embeds {tuple(embeds.shape)}, masks {tuple(masks.shape)}, {B} sequences, "
                             f"{n_patches} patches)")
        if n_patches + 1 + self.cfg["max_text_len"] > self.token_cap and self.dtype == L.BF16:
            raise self.token_limit_error(n_patches)
        if self._rank_pass is None:
            self._rank_pass = RankPass(self)
        rp = self._rank_pass.shape(B, n_patches)
        rp.text_ids = text_ids.to(self.device, torch.int64).contiguous()
        rp.text_mask = text_mask.to(self.device, torch.int64).contiguous()
        if tuple(rp.text_ids.shape) != (B, rp.d.L) or tuple(rp.text_mask.shape) != (B, rp.d.L):
            raise ValueError(f"rank_forward: text must be [B, max_text_len={rp.d.L}]")
        src = L.RankSrc(embeds=embeds.data_ptr(), masks=masks.data_ptr(), img_of=img_of.data_ptr(), n_img=n_img, ld_tok=ld_tok)
        tail = bool(cls_tail) and B <= 1024 and os.environ.get("RMCL_NO_CLS_TAIL", "0") != "1"
        fold = self.fold_of(False) if rp.dtype == L.BF16 else None
        check(lib.rmcl_encoder_forward_rank(C.byref(rp.d), L.MODE_INFER | (L.MODE_CLS_TAIL if tail else 0) | self.stream_bit(rp.d), P(self.q32), P(self.q_lp),
                                            P(rp.text_ids), P(rp.text_mask), C.byref(src), P(rp.co_mask), P(rp.workspace), P(rp.xn), fold,
                                            stream_ptr()), "encoder_forward_rank")
        rp.keep_alive = (embeds, masks, img_of)
        self.heads_forward(rp, key=False, want_q=False, wgrad=False)
        return rp

    def pgd_step(self, pb: PassBuffers, lr: float, eps: float, first: bool = False, out: torch.Tensor = None, sum_prev: bool = False):
        """delta <- clamp(delta + lr g / max|g|, +-eps) (pgd_attack_vilt.py:162-173).  ``out``: also written in the same pass,
        cast(patches32 + delta_new) = the next forward's operand (:144), or with ``sum_prev`` cast(patches32 + delta_old + delta_new) =
        the attacked view of objectives.py:176.  ``first``: the incoming delta is delta_0 = 0 and is not read (no zero fill)."""
        per = pb.d.P * pb.d.patch_k
        if out is None and not first:
            check(lib.rmcl_pgd_step(P(pb.gpatch), pb.dtype, P(pb.delta), P(pb.amax), pb.B, I64(per), F(lr), F(eps),
                                    stream_ptr()), "pgd_step")
            return
        flags = (L.PGD_DELTA_ZERO if first else 0) | (L.PGD_SUM_PREV if sum_prev else 0)
        odt = L.F32 if (out is not None and out.dtype == torch.float32) else L.BF16
        check(lib.rmcl_pgd_step_fused(P(pb.gpatch), pb.dtype, P(pb.delta), P(pb.amax), pb.B, I64(per), F(lr), F(eps), P(pb.patches32),
                                      P(out), odt, flags, stream_ptr()), "pgd_step_fused")

    # ---- PGD threat models (include/rmcl.h "PGD threat models", csrc/pgd_ball.hip) ----------------------------------------------
    def pgd_valid(self, pb: PassBuffers) -> torch.Tensor:
        """int32 [B]: the leading delta elements of each sample that belong to real patches (None: dense batch, all of them)"""
        if pb.geom is None:
            return None
        if getattr(pb, "_valid_of", None) is not pb.geom:                     # once per bound batch (a bind sets a new geometry object)
            pb._valid = (pb.geom.counts.to(torch.int64) * pb.d.patch_k).clamp_(max=pb.d.P * pb.d.patch_k).to(torch.int32)
            pb._valid_of = pb.geom
        return pb._valid

    @staticmethod
    def _box(box):
        return (0.0, 0.0) if box is None else (float(box[0]), float(box[1]))

    def pgd_step_ball(self, pb: PassBuffers, lr: float, eps: float, direction: int, ball: int, box=None, first: bool = False,
                      out: torch.Tensor = None, valid: torch.Tensor = None):
        """One step of a configured threat model on ``pb.gpatch``: delta <- project(delta + lr d) with d = g / max|g|, sign(g) or
        g / ||g||_2 and the L-inf or L2 ball of radius eps, then the pixel box (lo, hi) on patches32 + delta; ``out`` receives the cast of
        the boxed image in the same pass.  ``first``: the incoming delta is 0 and is not read.  ``valid``: int32 [B] valid element counts
        (default: the batch's ragged geometry); elements behind them keep delta 0.  There is no sum_prev form."""
        per = pb.d.P * pb.d.patch_k
        valid = self.pgd_valid(pb) if valid is None else valid
        lo, hi = self._box(box)
        odt = L.F32 if (out is not None and out.dtype == torch.float32) else L.BF16
        check(lib.rmcl_pgd_step_ball(P(pb.gpatch), pb.dtype, P(pb.delta), P(pb.ball), P(valid), pb.B, I64(per), F(lr), F(eps), int(direction), int(ball),
                                     F(lo), F(hi), P(pb.patches32), P(out), odt, L.PGD_DELTA_ZERO if first else 0, stream_ptr()), "pgd_step_ball")
        return out

    def pgd_random_start(self, pb: PassBuffers, eps: float, ball: int, seed: int, box=None, out: torch.Tensor = None, valid: torch.Tensor = None):
        """delta_0 of a random start into ``pb.delta`` - uniform in the L-inf cube, or on the L2 sphere, of radius eps, a pure function of
        (seed, sample index in the whole batch, element) - and cast(box(patches32 + delta_0)) into ``out`` (default ``pb.patchesT``),
        which is returned.  A lane draws what its samples would draw in the whole batch."""
        per = pb.d.P * pb.d.patch_k
        out = pb.patchesT if out is None else out
        valid = self.pgd_valid(pb) if valid is None else valid
        lo, hi = self._box(box)
        odt = L.F32 if out.dtype == torch.float32 else L.BF16
        check(lib.rmcl_pgd_random_start(P(pb.delta), P(pb.ball), P(valid), pb.B, I64(per), int(getattr(pb, "lane", 0)) * pb.B, int(seed) & 0xFFFFFFFF,
                                        F(eps), int(ball), F(lo), F(hi), P(pb.patches32), P(out), odt, stream_ptr()), "pgd_random_start")
        return out

    def pgd_keep_worst(self, score_new: torch.Tensor, best_score: torch.Tensor, best_restart: torch.Tensor, restart: int, delta: torch.Tensor,
                       best_delta: torch.Tensor, operand: torch.Tensor = None, best_operand: torch.Tensor = None, rows_per_decision: int = 1):
        """Worst case over restarts, decided on the device: decision j (``score_new[j]``, a 1-d view of any stride - a column of a task's
        row terms) takes restart `restart` iff restart == 0 or score_new[j] > best_score[j]; its rows_per_decision rows of delta /
        operand are then copied into best_delta / best_operand and best_score / best_restart updated.  No synchronisation."""
        D = int(best_score.numel())
        rows = D * rows_per_decision
        if score_new.dim() != 1 or score_new.numel() != D or score_new.dtype != torch.float32 or delta.numel() % max(rows, 1):
            raise L.RmclError("pgd_keep_worst: score_new must be a 1-d fp32 view with one entry per decision, delta [decisions * rows_per_decision, per]")
        odt = L.F32 if (operand is None or operand.dtype == torch.float32) else L.BF16
        check(lib.rmcl_pgd_keep_worst(P(score_new), I64(score_new.stride(0)), P(best_score), P(best_restart), int(restart), D, int(rows_per_decision),
                                      P(delta), P(best_delta), P(operand), P(best_operand), odt, I64(delta.numel() // max(rows, 1)), stream_ptr()),
              "pgd_keep_worst")

    def enqueue(self, keys_all: torch.Tensor, ptr: int):
        check(lib.rmcl_enqueue_f32(P(self.queue), P(keys_all), keys_all.shape[0], 128, I64(self.num_negative), I64(ptr),
                                   stream_ptr()), "enqueue")
