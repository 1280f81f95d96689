"""Objectives of the RMCL hot path.  Mirrors the free-function protocol of the reference's
vilt/modules/objectives.py (``compute_<task>(pl_module, batch) -> dict``); all tensor math runs in
librmcl_hip.so through ``pl_module.engine``."""
from __future__ import annotations

import os
from copy import copy

import torch

from ... import _lib as L
from ..._lib import lib, check, P, I64
from ...runtime import stream_ptr
from ...attack.pgd_attack_vilt import device_image
from ...task_loss import Nlvr2Pass, InfoNceLoss, BarlowLoss, VqaLoss, Nlvr2Loss
from . import dist_utils


class _DeferredBackward(torch.autograd.Function):
    """Gives a loss value computed by HIP kernels a ``.backward()``: the closure launches the HIP
    backward, which accumulates into the gradient arena that every ``param.grad`` is a view of."""

    @staticmethod
    def forward(ctx, anchor, value, closure, prescale=1.0):
        ctx.closure = closure
        ctx.prescale = float(prescale)
        return value.clone()

    @staticmethod
    def backward(ctx, grad_out):
        # data-parallel mean: the backward is linear in grad_out, so the 1/world_size of DDP's gradient averaging is applied
        # here (exact for power-of-two world sizes) and the collectives are plain SUMs - no pre-multiplied reduction op
        ctx.closure(grad_out * ctx.prescale if ctx.prescale != 1.0 else grad_out)
        return None, None, None, None


def _scalar(t):
    return t.reshape(())


def _loss_view(pl_module, loss, view, op, **hooks):
    """One loss view of an objective through its loss object (task_loss.py): forward on `op` (MODE_FULL where a gradient will be wanted);
    returns the loss value, whose backward runs loss -> head -> pooler -> encoder into the gradient arena, then ``after_backward``."""
    need_grad = torch.is_grad_enabled() and pl_module.training
    loss.forward(view, op, L.MODE_FULL if need_grad else L.MODE_INFER, want_grad=need_grad, defer=True, **hooks)
    value = loss.value
    if not need_grad:
        return value

    def backward(grad_out):
        loss.backward(view, op, L.MODE_FULL, g=grad_out)
        # one attacked view = one backward per step: its gradient all-reduces can start layer by layer right away
        # reduced over ranks once per step, after the step's last closure; a single closure (the image-view step) gets
        # per-layer all-reduces that start while the layers below are still in their backward
        pl_module.after_backward(overlap=True)

    return _DeferredBackward.apply(pl_module.grad_anchor, value, backward, pl_module.grad_prescale())


def _em(pl_module):
    """pl_module.epoch_metrics (vilt_utils.set_metrics): None on a model no trainer has taken - the objectives then queue nothing"""
    return getattr(pl_module, "epoch_metrics", None)


def _metric(pl_module, name):
    """The epoch-metric handle `name`, or None on a module without epoch metrics / without that attribute."""
    return getattr(pl_module, name, None) if _em(pl_module) is not None else None


def _feed_scalars(pl_module, phase, **values):
    """Scalar.update at the reference's call sites: `{phase}_{name}` <- value (a device scalar, or a host number as an immediate), then
    ONE rmcl_metrics_update for everything the objective queued."""
    em = _em(pl_module)
    if em is None:
        return
    for name, v in values.items():
        h = _metric(pl_module, f"{phase}_{name}")
        if h is not None:
            h.update(v)
    em.flush()


def _log_delta(pl_module, pb, task, phase):
    """compute_pgd's delta log (:184) of a single-image objective, from the patch-layout delta the attack left in `pb`"""
    pl_module.engine.delta_channel_norm(pb)
    # mean over ALL pixels of the (padded) batch image like torch.linalg.norm(delta, dim=1).mean() (:184); the pad pixels of
    # a zero-padded batch carry delta = 0 and are not stored in the patch layout
    n_pix = pb.delta.numel() // 3 if pb.geom is None else pb.B * pb.geom.shape[2] * pb.geom.shape[3]
    pl_module.log(f"{task}_attack/{phase}/delta", _scalar(pb.loss_sum / float(n_pix)))


def compute_pgd(pl_module, batch, loss_name, k_modality=None):
    """objectives.py:160-188 for loss_name == "moco"."""
    img_delta = pl_module.pgd_attacker.pgd_attack(pl_module, batch, k_modality=k_modality)
    batch["image"][0] = batch["image"][0] + img_delta                     # :176 (on top of img + delta_{K-1})
    phase = "train" if pl_module.training else "val"
    pl_module.log(f"{loss_name}_attack/{phase}/delta", torch.linalg.norm(img_delta, dim=1).mean())
    return batch


def compute_geometric(pl_module, batch, loss_name, k_modality=None):
    """objectives.py:190-215."""
    attack_words = pl_module.greedy_attacker.adv_attack_samples(pl_module, batch, k_modality)
    batch["text"] = attack_words["text"]
    batch["text_ids"] = attack_words["txt_input_ids"]
    batch["text_masks"] = attack_words["text_masks"]
    phase = "train" if pl_module.training else "val"
    pl_module.log(f"{loss_name}_attack/{phase}/num_changes", attack_words["num_changes"])
    pl_module.log(f"{loss_name}_attack/{phase}/change_rate", attack_words["change_rate"])
    batch["txt_attack_stats"] = (attack_words["num_changes"], attack_words["change_rate"])     # (host numbers: the epoch metrics' immediates)
    return batch


def _attacked_view(pl_module, pv, op, k, suffix, success_name, prediction_original, ret, phase, before_loss=None):
    """One loss view (objectives.py:287-317 / :324-354 / :362-392; suffix "clean": the clean query of :267-275 as a
    loss, BASELINE configs[1]): encoder forward on `op` with the text in `pv`, InfoNCE against the queue, metrics, and a
    loss tensor whose backward runs the HIP backward."""
    value = _loss_view(pl_module, InfoNceLoss(pl_module), pv, op, before_loss=before_loss, k=k)   # (before_loss: e.g. join the key-encoder stream)
    rows = pv.rows
    if phase == "train" and success_name is not None:
        pl_module.log(f"moco_attack/{success_name}", (rows[:, 1] != prediction_original).float().mean())
    means = rows.mean(dim=0)                           # one reduction launch for the six batch means (the values are views of it)
    for j, name in ((3, "pos_dist"), (4, "pos_cosine"), (5, "pos_dot"), (6, "neg_dist"), (7, "neg_cosine"), (8, "neg_dot")):
        ret[f"{name}_attacked_{suffix}"] = means[j]
    ret[f"q_{suffix}_attack"] = pv.q.clone()
    pl_module.log("moco_loss/clean_loss" if suffix == "clean" else f"moco_loss/attacked_{suffix}_loss", value.detach())
    return value


def compute_itm_wpa(pl_module, batch):
    """objectives.compute_itm_wpa (:714-787): ITM head + CE, and the word-patch-alignment OT distance
    (cosine cost :24-34, IPOT :46-76 with beta=0.5 / 50 iterations, trace :37-43)."""
    import ctypes as C
    from ..._lib import F
    eng = pl_module.engine
    dev = eng.device
    Bn = len(batch["text"])
    pos_len = Bn // 2
    itm_labels = torch.cat([torch.ones(pos_len), torch.zeros(Bn - pos_len)]).to(dev)
    forced = getattr(pl_module, "itm_labels_override", None)            # test hook: fix the 50/50 draw
    itm_labels = forced.to(dev).float() if forced is not None else itm_labels[torch.randperm(Bn, device=dev)]
    img, fimg = device_image(eng, batch["image"][0]), device_image(eng, batch["false_image_0"][0])   # the mix of the two views needs pixels
    images = torch.where(itm_labels.view(-1, 1, 1, 1) == 1, img, fimg)                 # :722-730

    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], images, tag="itm")
    d = pb.d
    Lt, Li, D = d.L, d.P + 1, d.D
    N = Lt + Li
    need_grad = torch.is_grad_enabled() and pl_module.training
    op = eng.make_operand(pb, out=pb.patchesT_full)
    eng.encoder_forward(pb, key=False, mode=L.MODE_FULL if need_grad else L.MODE_INFER, patchesT=op)
    eng.heads_forward(pb, key=False, want_q=False)
    st = stream_ptr()
    lay = eng.layout

    labels_i = itm_labels.to(torch.int32)
    logits = torch.empty(Bn, 2, device=dev)
    dlogits = torch.empty(Bn, 2, device=dev)
    losses = torch.zeros(2, device=dev)
    w_itm, b_itm = eng.q32[lay.itm_w:lay.itm_w + 2 * D], eng.q32[lay.itm_b:lay.itm_b + 2]
    check(lib.rmcl_itm_fwd(P(pb.cls), P(w_itm), P(b_itm), P(labels_i), P(logits), P(dlogits), P(losses), Bn, D, F(1.0 / Bn), st), "itm_fwd")

    # masks (:739-745): drop [CLS], the last valid text token and the image cls slot
    txt_mask = pb.text_mask.bool().clone()
    lens = txt_mask.sum(dim=1)
    txt_mask[torch.arange(Bn, device=dev), lens - 1] = False
    txt_mask[:, 0] = False
    img_mask = pb.co_mask[:, Lt:].bool().clone()
    img_mask[:, 0] = False
    txt_valid, img_valid = txt_mask.to(torch.int32).contiguous(), img_mask.to(torch.int32).contiguous()

    ld = (Li + 3) // 4 * 4
    M = Bn * N
    xhat, norms = torch.empty(M, D, device=dev), torch.empty(M, device=dev)
    check(lib.rmcl_l2norm_rows_fwd(P(pb.xn), P(xhat), P(norms), M, D, F(1e-5), st), "l2norm")
    cost = torch.zeros(Bn, Lt, ld, device=dev)
    img_rows = xhat[Lt:]                                                   # first image row of sample 0
    check(lib.rmcl_gemm_batched(P(xhat), P(img_rows), P(cost), Lt, Li, D, I64(D), I64(D), ld, F(1.0), Bn, I64(N * D), I64(N * D),
                                I64(Lt * ld), L.F32, L.F32, 1, 1, st), "cosine sim")
    check(lib.rmcl_wpa_cost_finish(P(cost), P(txt_valid), P(img_valid), Bn, Lt, Li, ld, st), "cost_finish")
    T = torch.empty(Bn, Li, Lt, device=dev)
    check(lib.rmcl_ipot_f32(P(cost), P(txt_valid), P(img_valid), P(T), Bn, Lt, Li, ld, F(0.5), 50, st), "ipot")
    w = (itm_labels * 2 - 1) * (0.1 / Bn)                                  # 0.1 * (sum_pos - sum_neg) / B  (:763-765,771)
    dist = torch.empty(Bn, device=dev)
    dsim = torch.empty(Bn, Lt, ld, device=dev) if need_grad else None
    check(lib.rmcl_wpa_distance(P(cost), P(T), P(w), P(dist), P(dsim), Bn, Lt, Li, ld, st), "wpa_distance")
    losses[1] = (dist * w).sum()
    value = losses.clone()

    if need_grad:
        def backward(grad_out, pb=pb, dlogits=dlogits, dsim=dsim, xhat=xhat, norms=norms, op=op):
            st2 = stream_ptr()
            g = grad_out.to(torch.float32)
            dl = dlogits * g[0]
            dcls_itm = torch.empty(Bn, D, device=dev)
            gw, gb = eng.g32[lay.itm_w:lay.itm_w + 2 * D], eng.g32[lay.itm_b:lay.itm_b + 2]
            if eng.irtr:
                # an IRTR model freezes itm_score (vilt_module.py:237-239): the ITM loss trains the encoder but writes no gradient into the
                # head - nor, through the alias, into rank_output
                gw = gb = None
            check(lib.rmcl_itm_bwd(P(dl), P(pb.cls), P(w_itm), P(dcls_itm), P(gw), P(gb), Bn, D, F(1.0), st2), "itm_bwd")
            eng.heads_backward(pb, None, dcls_itm, with_grads=True)
            ds = dsim * g[1]
            dxhat = torch.zeros(M, D, device=dev)
            check(lib.rmcl_gemm_batched(P(ds), P(xhat[Lt:]), P(dxhat), Lt, D, Li, I64(ld), I64(D), D, F(1.0), Bn, I64(Lt * ld),
                                        I64(N * D), I64(N * D), L.F32, L.F32, 1, 0, st2), "d txt")
            check(lib.rmcl_gemm_batched(P(ds), P(xhat), P(dxhat[Lt:]), Li, D, Lt, I64(ld), I64(D), D, F(1.0), Bn, I64(Lt * ld),
                                        I64(N * D), I64(N * D), L.F32, L.F32, 0, 0, st2), "d img")
            dxn = torch.empty(M, D, device=dev)
            check(lib.rmcl_l2norm_rows_bwd(P(dxhat), P(xhat), P(norms), P(dxn), M, D, st2), "l2norm_bwd")
            dxn.view(Bn, N, D)[:, 0] += pb.dcls
            eng.encoder_backward(pb, L.MODE_FULL, op, dxn, cls_only=False, dpatches=None)
            pl_module.after_backward()

        value = _DeferredBackward.apply(pl_module.grad_anchor, value, backward, pl_module.grad_prescale())
    ret = {"itm_loss": value[0], "itm_wpa_loss": value[1], "itm_logits": logits, "itm_labels": itm_labels}
    phase = "train" if pl_module.training else "val"
    pl_module.log(f"itm/{phase}/loss", ret["itm_loss"].detach())
    pl_module.log(f"itm/{phase}/wpa_loss", ret["itm_wpa_loss"].detach())
    pl_module.log(f"itm/{phase}/accuracy", (logits.argmax(-1) == itm_labels.long()).float().mean())
    if _em(pl_module) is not None:
        _metric(pl_module, f"{phase}_itm_accuracy").update(logits, labels_i)
        _feed_scalars(pl_module, phase, itm_loss=value[0].detach(), itm_wpa_loss=value[1].detach())
    return ret


def _pred_head_backward(pl_module, value, pb, op, head_backward, replaced=None):
    """Gives the loss of a prediction head (MLM, MPP) its ``.backward()``: the head's backward (``head_backward(g, dxn)``: Engine.mlm_backward /
    mpp_backward on the incoming gradient g [1] and a zero-filled dxn [B N, D]), then the full-row encoder backward and the step's
    gradient reduction."""
    eng = pl_module.engine
    rows = pb.B * (pb.d.L + 1 + pb.d.P)

    def backward(grad_out):
        g = grad_out.to(torch.float32).reshape(1).contiguous()
        dxn = torch.zeros(rows, pb.d.D, dtype=torch.float32, device=eng.device)
        head_backward(g, dxn)
        eng.encoder_backward(pb, L.MODE_FULL, op, dxn, cls_only=False, dpatches=None, replaced=replaced)
        pl_module.after_backward()

    return _DeferredBackward.apply(pl_module.grad_anchor, value, backward, pl_module.grad_prescale())


def _pred_head_report(pl_module, task, value, stats):
    """What compute_mlm and compute_mpp do with stats = (loss, correct, labelled) once the loss stands - Accuracy (gadgets/my_metrics.py:5-28):
    correct / total over the labelled rows (MPP: (row, channel) pairs), per step and accumulated over the epoch; the two logs; the epoch
    metrics."""
    phase = "train" if pl_module.training else "val"
    acc = getattr(pl_module, f"{task}_epoch_counts", None)
    if acc is None:
        acc = {}
        setattr(pl_module, f"{task}_epoch_counts", acc)
    if phase not in acc:
        acc[phase] = torch.zeros(2, dtype=torch.float32, device=stats.device)
    acc[phase] += stats[1:3]
    pl_module.log(f"{task}/{phase}/loss", value.detach())
    pl_module.log(f"{task}/{phase}/accuracy", stats[1] / stats[2])
    if _em(pl_module) is not None:
        # (a batch without a labelled row has a NaN loss, here as in the reference; gated on the row count it leaves the epoch loss alone)
        _metric(pl_module, f"{phase}_{task}_accuracy").update_counts(stats[1:2], stats[2:3])
        _metric(pl_module, f"{phase}_{task}_loss").update(value.detach(), gate=stats[2:3])
        _em(pl_module).flush()


def compute_mlm(pl_module, batch):
    """objectives.compute_mlm (:604-630): one FULL-mode encoder pass on the masked ids (no cls-only tail: the loss reads text rows), then
    mlm_score and the cross-entropy over the positions whose label is not -100 - on those rows only, compacted, with the decoder and
    the softmax fused (csrc/mlm.hip): no [B, L, vocab] logits tensor exists on the training path.  ``mlm_logits`` is the dense tensor
    when config["mlm_return_logits"] is true or the call runs under no_grad in eval mode, else None (INTEGRATION.md "MLM")."""
    eng = pl_module.engine
    cfg = pl_module.hparams.config
    if eng.mlm is None:
        raise ValueError("compute_mlm needs a model built with loss_names['mlm'] > 0 (the mlm_score head)")
    need_grad = torch.is_grad_enabled() and pl_module.training
    ids, labels = batch["text_ids_mlm"], batch["text_labels_mlm"]
    pb = eng.bind_batch(ids, batch["text_masks"], batch["image"][0], tag="mlm")
    d = pb.d
    N = d.L + 1 + d.P
    mb = eng.mlm_bind(eng.mlm_bufs(pb.B, "mlm"), labels, N)                 # (validates the labels before anything is launched on them)
    op = eng.make_operand(pb, out=pb.patchesT_full)
    eng.encoder_forward(pb, key=False, mode=L.MODE_FULL if need_grad else L.MODE_INFER, patchesT=op)
    stats = eng.mlm_forward(mb, pb.xn)                                      # (loss, correct rows, rows with a label), all on the device
    value = _scalar(stats[0:1].clone())
    if need_grad:
        value = _pred_head_backward(pl_module, value, pb, op, lambda g, dxn: eng.mlm_backward(mb, 1.0, g, dxn, with_grads=True))
    logits = None
    if cfg.get("mlm_return_logits", False) or not (torch.is_grad_enabled() or pl_module.training):
        ma = eng.mlm_bind(eng.mlm_bufs(pb.B, "mlm_dense"), labels, N, all_rows=True)
        eng.mlm_forward(ma, pb.xn)
        logits = eng.mlm_logits(ma, ma.M).view(pb.B, d.L, eng.mlm.V)
    _pred_head_report(pl_module, "mlm", value, stats)
    return {"mlm_loss": value, "mlm_logits": logits, "mlm_labels": labels, "mlm_ids": ids}


def _mpp_pass(pl_module, batch, text_ids, tag, mode):
    """The masked-image encoder pass shared by compute_mpp and infer(mask_image=True): the image on the device (float, or the bytes of a
    Uint8Batch / RawUint8Batch), the two mask draws
    (batch["mpp_masked"] / ["mpp_replaced"] [B, G] bool replace them) BEFORE the patch selection's own draws - the reference's order
    (vision_transformer.py:602-603 before :632-645) -, the labels and the compaction, then the encoder forward with the mask-token
    substitution.  Returns (pb, mp, op, img)."""
    from ...runtime import mpp_draw_masks
    eng = pl_module.engine
    if eng.mpp is None:
        raise NotImplementedError("MPP masking (mask_image=True / compute_mpp) needs a model built with loss_names['mpp'] > 0 "
                                  "(transformer.mask_token and the mpp_score head)")
    image = batch["image"][0]
    if torch.is_tensor(image):
        img = image.to(eng.device, torch.float32).contiguous()
    else:
        # byte feeds (Uint8Batch; a RawUint8Batch is resized on the device first): the patch rows AND the labels come from the bytes
        # (rmcl_image_u8_to_patches, rmcl_mpp_labels_u8) - no float image exists on this path
        img = eng.u8_on_device(image)
    B, _, Hh, Ww = img.shape
    ps = int(pl_module.hparams.config["patch_size"])
    G = (Hh // ps) * (Ww // ps)
    if "mpp_masked" in batch and "mpp_replaced" in batch:
        masked, replaced = batch["mpp_masked"].bool(), batch["mpp_replaced"].bool()
    else:
        masked, replaced = mpp_draw_masks(B, G)
    pb = eng.bind_batch(text_ids, batch["text_masks"], img, tag=tag)
    mp = eng.mpp_bind(eng.mpp_bufs(pb.B, tag, pb.d.P), img, pb, masked, replaced)
    eng.mpp_check_labels(mp)
    op = eng.make_operand(pb, out=pb.patchesT_full)
    eng.encoder_forward(pb, key=False, mode=mode, patchesT=op, replaced=mp.replaced)
    return pb, mp, op, img


def mpp_image_labels(mp) -> torch.Tensor:
    """image_labels [B, 1 + P, 3] int64 with the reference's meaning (vision_transformer.py:549, 653-659): the label of every masked
    valid slot, -100 everywhere else and in the prepended cls row."""
    lab = torch.where(mp.masked.bool().unsqueeze(-1), mp.labels, torch.full_like(mp.labels, -100)).to(torch.int64)
    return torch.cat([torch.full((mp.B, 1, 3), -100, dtype=torch.int64, device=lab.device), lab], dim=1)


def compute_mpp(pl_module, batch):
    """objectives.compute_mpp (:632-665): one FULL-mode encoder pass with masked patches (no cls-only tail: the loss reads image rows),
    then mpp_score and three 256-way cross-entropies per masked valid slot - on those rows only, compacted (csrc/mpp.hip).
    ``mpp_logits`` [B, 1 + P, 3, 256] is the dense tensor when config["mpp_return_logits"] is true or the call runs under no_grad in
    eval mode, else None (INTEGRATION.md "MPP")."""
    eng = pl_module.engine
    cfg = pl_module.hparams.config
    need_grad = torch.is_grad_enabled() and pl_module.training
    pb, mp, op, img = _mpp_pass(pl_module, batch, batch["text_ids"], "mpp", L.MODE_FULL if need_grad else L.MODE_INFER)
    d = pb.d
    stats = eng.mpp_forward(mp, pb.xn)                                      # (loss, correct pairs, labelled pairs), all on the device
    value = _scalar(stats[0:1].clone())
    if need_grad:
        value = _pred_head_backward(pl_module, value, pb, op, lambda g, dxn: eng.mpp_backward(mp, 1.0, g, dxn, with_grads=True),
                                    replaced=mp.replaced)
    labels = mpp_image_labels(mp)
    logits = None
    if cfg.get("mpp_return_logits", False) or not (torch.is_grad_enabled() or pl_module.training):
        ma = eng.mpp_bufs(pb.B, "mpp_dense", d.P)
        ma.labels.copy_(mp.labels)
        ma.masked, ma.replaced = mp.masked, mp.replaced
        eng.mpp_compact(ma, pb, all_rows=True)
        eng.mpp_forward(ma, pb.xn)
        logits = eng.mpp_logits(ma, pb.B * (d.P + 1)).view(pb.B, d.P + 1, 3, 256)
    _pred_head_report(pl_module, "mpp", value, stats)
    return {"mpp_loss": value, "mpp_logits": logits, "mpp_labels": labels}


def compute_moco_contrastive(pl_module, batch):
    """objectives.py:217-447 (image view).  Returns {"moco_loss", pos_/neg_{dist,cosine,dot}_attacked_img}."""
    eng = pl_module.engine
    clean_view = bool(pl_module.hparams.config.get("clean_view", False))
    if not (pl_module.image_view or pl_module.text_view or clean_view):
        raise ZeroDivisionError("division by zero: loss / loss_num with both views off (objectives.py:250-251,397)")
    if pl_module.augmentation:
        raise NotImplementedError("augmentation views are out of scope (SURVEY 2.1 #17)")
    phase = "train" if pl_module.training else "val"
    ret = {}

    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0])
    B = pb.B

    op = eng.make_operand(pb)
    # The momentum-encoder forward (infer_k under no_grad, :262-265) and the clean query forward (:267-275)
    # are independent: they run on two HIP streams so each fills the other's tile-quantisation tails.
    pk = eng.twin(pb, "key")
    pk.text_ids, pk.text_mask = pb.text_ids, pb.text_mask
    pk.k = pb.k                            # the key head writes the keys where the query passes read them (no copy launch after the join)
    main = torch.cuda.current_stream()
    side = eng.side_stream
    if eng.lp_stale:                       # (after a checkpoint load / manual weight edit) refresh the bf16 shadows on the MAIN
        eng.refresh_shadows()              # stream before forking: both streams read them
    # momentum update (:257-260).  (Moving the 1.6 GB sweep onto the key encoder's stream, beside the query encoder's first
    # forward, measured no gain: 37.5 vs 37.6 ms per step - both are HBM-bound there.)
    eng.ema(pl_module.momentum)
    # PGD step 0 runs the query encoder on img + delta_0 = img: with dropout off that IS the clean query forward
    # (:267-275), so it is computed once (common sub-expression) and its logits give prediction_original.
    # Under dropout the reference draws a fresh mask for the clean forward (:267) and another for PGD step 0's (pgd_attack_vilt.py:145), so
    # the two are different computations and both run.  config["share_clean_forward"] = True (default False) lets PGD step 0's forward stand in
    # for the clean one under dropout too: loss, gradients and the perturbation are untouched (the clean logits never enter the loss,
    # SURVEY quirk 3) - only the LOGGED prediction_original / q_original then come from the forward that shares step 0's mask.
    share = bool(pl_module.hparams.config.get("share_clean_forward", False))
    fuse_clean = pl_module.image_view and not pl_module.text_view and (not eng.dropout_on or share) and not clean_view
    # two half-batch chains (Engine.lanes) where the PGD loop is the step's front: each lane runs its own K iterations, lane 0 on this
    # stream, lane 1 on the side stream.  With dropout ON the clean query forward cannot be shared with PGD step 0 (the reference draws
    # a fresh mask for each, objectives.py:267 vs pgd_attack_vilt.py:145): it then follows the key forward on the key stream, in its own
    # buffers, beside the lanes
    use_lanes = (pl_module.image_view and not pl_module.text_view and not clean_view and eng.pgd_bufs(pb) is pb and eng.lanes(pb) is not None)
    # with the lanes on this stream and the side stream, the key forward takes the (idle) weight-gradient stream: three chains
    key_stream = eng.dw_stream if (use_lanes and (os.environ.get("RMCL_KEY_LANES", "0") != "1" or not fuse_clean)) else side
    key_lanes = eng.lanes(pk) if (use_lanes and key_stream is side) else None
    k_ready = None                          # event: the keys are in pb.k (None: wait for the whole key stream)
    if key_lanes is not None:
        eng.fold_of(True)                                   # (refreshed on the main stream before the fork)
        side.wait_stream(main)
        check(lib.rmcl_tune_set(10, len(key_lanes)), "tune_set")
        try:
            per = key_lanes[0].B * pb.d.P
            for i, kl in enumerate(key_lanes):
                with torch.cuda.stream(side if i else main):
                    eng.encoder_forward(kl, key=True, mode=L.MODE_INFER, patchesT=op[i * per:(i + 1) * per], cls_tail=True)
                    eng.heads_forward(kl, key=True, wgrad=False)
        finally:
            check(lib.rmcl_tune_set(10, 1), "tune_set")      # (process-global routing state: restored on every path)
    else:
        if use_lanes and not fuse_clean:
            eng.fold_of(False)                              # the clean query pass will read the query fold on the key stream: refresh it before the fork
        key_stream.wait_stream(main)
        with torch.cuda.stream(key_stream):
            eng.encoder_forward(pk, key=True, mode=L.MODE_INFER, patchesT=op, cls_tail=True)
            eng.heads_forward(pk, key=True, wgrad=False)
            k_ready = torch.cuda.Event()
            k_ready.record(key_stream)
    gather_box = {}

    def join_key_stream():
        if k_ready is not None:
            main.wait_event(k_ready)
        else:
            main.wait_stream(key_stream)
        # asynchronous key all-gather (RCCL's own stream): overlaps everything until the enqueue (one rank: the keys themselves)
        gather_box["g"] = dist_utils.KeyGather(pb.k.clone() if dist_utils.world_size() > 1 else pb.k) if pl_module.training else None

    k = pb.k
    clean = {}
    clean_on_key = False
    loss = 0
    loss_num = 0
    if clean_view:
        # build extension (config key "clean_view", default off): CE on the clean logits of :267-275 as a loss term -
        # BASELINE configs[1] "clean ITM + contrastive" (SURVEY 8d Config 2).  The reference forms these logits in
        # every step but never turns them into a loss (quirk 3).
        pc = eng.bind_text(pb, pb.text_ids, pb.text_mask, tag="moco_clean")
        op_c = eng.make_operand(pb, out=pc.patchesT_full)
        loss = loss + _attacked_view(pl_module, pc, op_c, k, "clean", None, None, ret, phase, before_loss=join_key_stream)
        clean = {"prediction": pc.rows[:, 1].clone(), "q": pc.q.clone()}
        loss_num += 1
    elif not fuse_clean and use_lanes and k_ready is not None:
        # clean query (:267-275) behind the key forward on the key stream, in buffers of its own (the lanes' passes use pb's)
        pc = eng.twin(pb, "clean_q")
        pc.text_ids, pc.text_mask, pc.k = pb.text_ids, pb.text_mask, pb.k
        clean = {"prediction": torch.empty(B, dtype=torch.float32, device=eng.device), "q": torch.empty_like(pb.q)}
        with torch.cuda.stream(key_stream):
            InfoNceLoss(pl_module, metrics=False).forward(pc, op, L.MODE_INFER, want_grad=False, scale=0.0, wgrad=False)
            clean["prediction"].copy_(pc.rows[:, 1])
            clean["q"].copy_(pc.q)
        clean_on_key = True
    elif not fuse_clean:
        InfoNceLoss(pl_module, metrics=False).forward(pb, op, L.MODE_INFER, want_grad=False, scale=0.0, before_loss=join_key_stream, clean_out=clean)   # clean query
    prediction_original = clean.get("prediction")

    txt_ids = txt_masks = None
    if pl_module.text_view:                                                 # :277-317
        aug = compute_geometric(pl_module, copy(batch), "moco", k_modality=k)
        txt_ids, txt_masks = aug["text_ids"], aug["text_masks"]
        pt = eng.bind_text(pb, txt_ids, txt_masks, tag="moco_txt")
        op_t = eng.make_operand(pb, out=pt.patchesT_full)                   # clean image, attacked text
        loss = loss + _attacked_view(pl_module, pt, op_t, k, "txt", "Geom_success_rate", prediction_original, ret, phase)
        loss_num += 1
    if pl_module.image_view:                                                # :319-354
        if key_lanes is not None:
            join_key_stream()                               # lane 0 waits for lane 1's key forward only; every lane reads its own keys
            pl_module.pgd_attacker.attack_patches(pl_module, pb, None, clean_out=clean, clean_op=op)
            prediction_original = clean["prediction"]
        elif fuse_clean:
            pl_module.pgd_attacker.attack_patches(pl_module, pb, None, before_first_loss=join_key_stream, clean_out=clean, clean_op=op,
                                                  key_stream=key_stream, key_event=k_ready)
            prediction_original = clean["prediction"]
        elif clean_on_key:
            pl_module.pgd_attacker.attack_patches(pl_module, pb, None, before_first_loss=join_key_stream, clean_op=op, key_stream=key_stream,
                                                  key_event=k_ready)
            main.wait_stream(key_stream)                    # the clean query's prediction / q (key stream) are read from here on
        else:
            pl_module.pgd_attacker.attack_patches(pl_module, pb, k, clean_op=op)        # compute_pgd (:319-323)
        _log_delta(pl_module, pb, "moco", phase)
        # attacked view = img + delta_{K-1} + delta_K  (pgd_attack_vilt.py:144 + objectives.py:176): written by the last PGD update
        op_att = pb.patchesT_full
        loss_i = _attacked_view(pl_module, pb, op_att, k, "img", "PGD_success_rate", prediction_original, ret, phase)
        ret["logit_pos_img_attack"] = pb.rows[:, 2].clone()
        ret["lse_img_attack"] = pb.rows[:, 9].clone()
        loss = loss + loss_i
        loss_num += 1
    if pl_module.image_view and pl_module.text_view:                        # :356-392 attacked image AND attacked text
        pbo = eng.bind_text(pb, txt_ids, txt_masks, tag="moco_both")
        op_b = pbo.patchesT_full.copy_(pb.patchesT_full)                    # the same attacked image (own buffer: read again by the backward)
        loss = loss + _attacked_view(pl_module, pbo, op_b, k, "both", "Both_success_rate", prediction_original, ret, phase)
        loss_num += 1

    if pl_module.training:                                                  # _dequeue_and_enqueue (:394-395)
        keys_all = gather_box["g"].wait()
        do, new_ptr = dist_utils.queue_advance(pl_module.queue_ptr, keys_all.shape[0], pl_module.num_negative,
                                               pl_module.per_step_bs)
        if do:
            eng.enqueue(keys_all, pl_module.queue_ptr)
            pl_module.queue_ptr = new_ptr

    ret["moco_loss"] = loss / loss_num
    ret["k"] = k.clone()
    ret["q_original"] = clean["q"]
    pl_module.log(f"moco_loss/step/{phase}", ret["moco_loss"].detach())
    _feed_scalars(pl_module, phase, moco_loss=ret["moco_loss"].detach())
    views = (["img"] if pl_module.image_view else []) + (["txt"] if pl_module.text_view else []) + \
            (["both"] if pl_module.image_view and pl_module.text_view else [])
    for v in views:                                                         # :402-445
        for kind, tag in (("dist", "L2"), ("cosine", "Cosine"), ("dot", "Dot")):
            pos, neg = ret[f"pos_{kind}_attacked_{v}"], ret[f"neg_{kind}_attacked_{v}"]
            pl_module.log(f"moco_dist_{phase}_{tag}/Pos_attacked_{v}", pos)
            pl_module.log(f"moco_dist_{phase}_{tag}/Neg_attacked_{v}", neg)
            pl_module.log(f"moco_dist_{phase}_{tag}/Neg-Pos_attacked_{v}", neg - pos)
    return ret


def _bt_view(pl_module, pv, op, zk, suffix, name, ret, views, need_grad, training):
    """One Barlow-Twins loss view (objectives.py:464-498 text / :500-525 image / :527-546 both): forward of the view, the
    head (running estimates updated in training), c = q^T k / per_step_bs summed over ranks, on/off-diagonal loss, distance
    logs; returns the loss value with a deferred HIP backward; on_diag and adv_lr * off_diag go into `ret` under `name`."""
    def reduce_c(c):                                                            # torch.distributed.all_reduce(c) (:480,:507,:535)
        if dist_utils.world_size() > 1:
            torch.distributed.all_reduce(c)

    # NOTE on ranks: the reference all-reduces c WITHOUT autograd support, so each rank backpropagates d loss(c_global) / dq
    # of its own rows and DDP then AVERAGES the gradients - the 1/world_size of that average is the prescale
    loss = BarlowLoss(pl_module, "q_" + suffix, zk, track=training, denom=pl_module.per_step_bs, reduce_c=reduce_c)
    value = _loss_view(pl_module, loss, pv, op)
    on_diag, red = loss.on_diag, loss.red
    rows = pl_module.engine.bt_pair_metrics(loss.bb, zk)
    ret[f"pos_dist_attacked_{suffix}"], ret[f"pos_cosine_attacked_{suffix}"], ret[f"pos_dot_attacked_{suffix}"] = \
        rows[:, 0].mean(), rows[:, 1].mean(), rows[:, 2].mean()
    ret[f"q_{suffix}"] = loss.bb.z.clone()
    if need_grad:
        # Reference behaviour: training_step sums every returned value whose key contains "loss" (vilt_module.py:475), and the
        # logged components ARE live graph tensors there (:486-487) - each view is optimised with weight 1/loss_num + 1.  The
        # invariance component therefore carries the same deferred backward (as a zero-valued term).
        on_diag = on_diag + (value - value.detach())
    ret[f"barlowtwins_loss_invariance_{name}"], ret[f"barlowtwins_loss_redundancy_{name}"] = on_diag, red
    views.append((suffix, name))
    return value


def compute_barlowtwins_contrastive(pl_module, batch):
    """objectives.py:449-602: ONE encoder and one head.  k = head(infer(clean)) under no_grad; per view
    q = head(infer(view)), c = q^T k / per_step_bs summed over ranks, loss = sum_i (c_ii - 1)^2 + adv_lr * sum_{i != j} c_ij^2
    (the reference uses its `adv_lr` hyper-parameter as the redundancy weight).  Views like the MoCo objective: attacked text
    (greedy attack on this loss), attacked image (PGD on this loss; img + delta_{K-1} + delta_K), both.  The head's BatchNorms
    run in the module's mode and - in training - update their running estimates in EVERY call, also under no_grad."""
    eng = pl_module.engine
    if pl_module.augmentation:
        raise NotImplementedError("augmentation views are out of scope (SURVEY 2.1 #17)")
    if not (pl_module.image_view or pl_module.text_view):
        raise ZeroDivisionError("division by zero: loss / loss_num with both views off (objectives.py:451-452,548)")
    phase = "train" if pl_module.training else "val"
    training = bool(pl_module.training)
    need_grad = torch.is_grad_enabled() and training
    ret = {}
    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0], tag="bt")
    B = pb.B
    op = eng.make_operand(pb)
    key = BarlowLoss(pl_module, "k", track=training)
    eng.encoder_forward(pb, key=False, mode=L.MODE_INFER, patchesT=op, cls_tail=True)          # :460-462
    key.pool(pb, True)
    zk = key.project(pb, pb.cls)
    loss, loss_num = 0, 0
    views = []
    txt_ids = txt_masks = None
    if pl_module.text_view:                                                     # :464-498
        aug = compute_geometric(pl_module, copy(batch), "barlowtwins", k_modality=zk)
        txt_ids, txt_masks = aug["text_ids"], aug["text_masks"]
        pt = eng.bind_text(pb, txt_ids, txt_masks, tag="bt_txt")
        op_t = eng.make_operand(pb, out=pt.patchesT_full)
        loss, loss_num = loss + _bt_view(pl_module, pt, op_t, zk, "txt", "text", ret, views, need_grad, training), loss_num + 1
    if pl_module.image_view:                                                    # :500-525
        pl_module.pgd_attacker.attack_patches(pl_module, pb, zk, clean_op=op)   # compute_pgd (:503)
        _log_delta(pl_module, pb, "barlowtwins", phase)
        op_att = pb.patchesT_full                                               # written by the last PGD update
        loss, loss_num = loss + _bt_view(pl_module, pb, op_att, zk, "img", "img", ret, views, need_grad, training), loss_num + 1
    if pl_module.image_view and pl_module.text_view:                            # :527-546
        pbo = eng.bind_text(pb, txt_ids, txt_masks, tag="bt_both")
        op_b = pbo.patchesT_full.copy_(pb.patchesT_full)
        loss, loss_num = loss + _bt_view(pl_module, pbo, op_b, zk, "both", "both", ret, views, need_grad, training), loss_num + 1
    ret["k"] = zk.clone()
    ret["barlowtwins_loss"] = loss / loss_num                                   # :548
    pl_module.log(f"barlowtwins/{phase}/loss", ret["barlowtwins_loss"].detach())
    if _em(pl_module) is not None:
        parts = {f"barlowtwins_loss_{part}_{name}": ret[f"barlowtwins_loss_{part}_{name}"].detach()
                 for _, name in views for part in ("invariance", "redundancy")}
        _feed_scalars(pl_module, phase, barlowtwins_loss=ret["barlowtwins_loss"].detach(), **parts)
    for suffix, name in views:                                                  # :555-600
        pl_module.log(f"barlowtwins_dist_{phase}_L2/Pos_attacked_{suffix}", ret[f"pos_dist_attacked_{suffix}"])
        pl_module.log(f"barlowtwins_dist_{phase}_Cosine/Pos_attacked_{suffix}", ret[f"pos_cosine_attacked_{suffix}"])
        pl_module.log(f"barlowtwins_dist_{phase}_Dot/Pos_attacked_{suffix}", ret[f"pos_dot_attacked_{suffix}"])
        pl_module.log(f"barlowtwins/{phase}/barlowtwins_loss_invariance_{name}", ret[f"barlowtwins_loss_invariance_{name}"].detach())
        pl_module.log(f"barlowtwins/{phase}/barlowtwins_loss_redundancy_{name}", ret[f"barlowtwins_loss_redundancy_{name}"].detach())
    return ret


def _vqa_head_loss(pl_module, pb, op, batch, task, vb_tag, tables=None):
    """Encoder forward of the view in `op`, pooler, vqa_classifier and the soft-target BCE (objectives.py:813-896): returns the
    reference's dict with a ``vqa_loss`` whose backward runs BCE gradient -> head -> pooler -> encoder (MODE_FULL) into the
    gradient arena.  ``tables``: VqaBuffers whose label / score tables this batch already sent (the PGD loop's)."""
    eng = pl_module.engine
    vb = eng.vqa_bufs(pb.B, vb_tag)

    bind = (lambda: eng.vqa_targets(vb, batch["vqa_labels"], batch["vqa_scores"])) if tables is None else \
        (lambda: vars(vb).update(labels=tables.labels, scores=tables.scores, A=tables.A))
    loss = VqaLoss(pl_module, vb)
    value, logits, loss2 = _loss_view(pl_module, loss, pb, op, before_loss=bind), loss.logits, loss.stats
    ret = {
        "vqa_loss": value,
        "vqa_logits": logits,
        "vqa_targets": eng.vqa_targets_dense(vb),
        "vqa_labels": batch["vqa_labels"],
        "vqa_scores": batch["vqa_scores"],
        "vqa_preds": vb.argmax,                     # (first maximum of the logits: what VQAScore and vqa_test_step read)
    }
    phase = "train" if pl_module.training else "val"
    pl_module.log(f"{task}/{phase}/loss", value.detach())
    pl_module.log(f"{task}/{phase}/score", loss2[1])
    if _em(pl_module) is not None:
        # VQAScore.update: rows[b][1] of rmcl_vqa_bce IS the soft target at sample b's first maximum
        _metric(pl_module, f"{phase}_{task}_score").update(vb.rows[:, 1], pb.B, stride=2)
        _feed_scalars(pl_module, phase, **{f"{task}_loss": value.detach()})
    return ret


def compute_vqa(pl_module, batch):
    """objectives.py:861-896: vqa_classifier on the pooler output of the clean batch, BCE-with-logits x vqav2_label_size."""
    eng = pl_module.engine
    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0], tag="vqa")
    op = eng.make_operand(pb, out=pb.patchesT_full)
    return _vqa_head_loss(pl_module, pb, op, batch, "vqa", "vqa")


def compute_vqa_attack(pl_module, batch):
    """objectives.py:813-859.  Image view: PGD on the VQA loss (PGDAttack_vqa, through compute_pgd's img + delta_{K-1} + delta_K).
    Text view: GreedyAttack_vqa on the CLEAN image (compute_geometric on a deepcopy of the batch, :820).  The head and the loss then run
    on (attacked or clean image, attacked or clean text); with both views the attacked sentence is paired with the attacked image
    (:821-823).  The batch itself is not modified (the reference attacks deep copies)."""
    eng = pl_module.engine
    phase = "train" if pl_module.training else "val"
    pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0], tag="vqa_att")
    vp = eng.vqa_targets(eng.vqa_bufs(pb.B, "pgd"), batch["vqa_labels"], batch["vqa_scores"])
    if pl_module.image_view:
        op = eng.make_operand(pb)                                             # img + delta_0, delta_0 = 0
        pl_module.pgd_attacker.attack_patches(pl_module, pb, vp, clean_op=op)    # compute_pgd (:816)
        _log_delta(pl_module, pb, "vqa_attacked", phase)
        op = pb.patchesT_full
    else:
        op = eng.make_operand(pb, out=pb.patchesT_full)                       # the clean image, built once
    if pl_module.text_view:
        aug = compute_geometric(pl_module, copy(batch), "vqa_attacked")       # (:820) on the clean image
        pb.text_ids = aug["text_ids"].to(eng.device, torch.int64).contiguous()
        pb.text_mask = aug["text_masks"].to(eng.device, torch.int64).contiguous()
    return _vqa_head_loss(pl_module, pb, op, batch, "vqa_attacked", "vqa_att", tables=vp)


# ---- NLVR2 (objectives.py:898-1060) ------------------------------------------------------------------------------------------------
def _nlvr2_loss(pl_module, npass, batch, nb_tag, labels_from=None, ref=None):
    """Forward of the pass on its operands, nlvr2_classifier and the CE: (value with a deferred backward, logits, Nlvr2Buffers, stats)."""
    eng = pl_module.engine
    nb = eng.nlvr2_bufs(npass.B, nb_tag)
    loss = Nlvr2Loss(pl_module, nb, ref)
    bind = (lambda: eng.nlvr2_labels(nb, batch["answers"])) if labels_from is None else (lambda: nb.labels.copy_(labels_from.labels))
    value = _loss_view(pl_module, loss, npass, None, before_loss=bind)
    return value, loss.logits, nb, loss.stats


def _split_rows(batch):
    """dev / test rows of a validation batch (objectives.py:1036-1037, selected by table_name)"""
    names = batch.get("table_name", [])
    return {"dev": [i for i, n in enumerate(names) if "dev" in n], "test": [i for i, n in enumerate(names) if "test" in n]}


def _log_split(pl_module, batch, task, nb, ref_nb=None):
    dev = nb.rows.device
    for split, idx in _split_rows(batch).items():
        if not idx:
            continue
        ix = torch.tensor(idx, dtype=torch.int64, device=dev)
        pl_module.log(f"{task}/{split}/loss", nb.rows.index_select(0, ix).mean())
        pl_module.log(f"{task}/{split}/accuracy", (nb.argmax.index_select(0, ix) == nb.labels.index_select(0, ix)).float().mean())
        if ref_nb is not None:                                               # change_rate (my_metrics.py:30-45): attacked vs clean argmax
            pl_module.log(f"{task}/{split}/change_rate_cross",
                          (nb.argmax.index_select(0, ix) != ref_nb.argmax.index_select(0, ix)).float().mean())


def _split_groups(batch, device):
    """the group table of a validation batch for the grouped metric ops: 0 = dev, 1 = test, -1 = neither; built once per batch.  (A name
    with both words would sit in both of the reference's lists; no table of the NLVR2 datasets has one, and dev wins here.)"""
    names = batch.get("table_name", [])
    return torch.tensor([0 if "dev" in n else (1 if "test" in n else -1) for n in names], dtype=torch.int32).to(device, non_blocking=True)


def _feed_split(pl_module, task, nb, group, ref_nb=None):
    """Validation metrics of one NLVR2 pass by split: the mean CE of the split's rows (Scalar), its accuracy, and - against `ref_nb` - the
    rate of changed predictions; dev and test in one grouped op each."""
    em = pl_module.epoch_metrics
    B = int(nb.rows.shape[0])
    em.rowmean([f"dev_{task}_loss", f"test_{task}_loss"], nb.rows, B, group=group)
    em.match([f"dev_{task}_accuracy", f"test_{task}_accuracy"], nb.argmax, nb.labels, B, group=group)
    if ref_nb is not None:
        em.match([f"dev_{task}_change_rate_cross", f"test_{task}_change_rate_cross"], nb.argmax, ref_nb.argmax, B, invert=True, group=group)


def compute_nlvr2(pl_module, batch):
    """objectives.py:1002-1060: CE(nlvr2_classifier(cat(cls(image_0, type 1), cls(image_1, type 2))), answers)."""
    eng = pl_module.engine
    npass = Nlvr2Pass.bind(pl_module, batch, "nlvr2")
    npass.clean_operands()
    value, logits, nb, stats = _nlvr2_loss(pl_module, npass, batch, "nlvr2")
    ret = {"nlvr2_loss": value, "nlvr2_logits": logits, "nlvr2_labels": nb.labels.to(torch.int64)}
    if pl_module.training:
        pl_module.log("nlvr2/train/loss", value.detach())
        pl_module.log("nlvr2/train/accuracy", _scalar(stats[1]) / float(npass.B))
        if _em(pl_module) is not None:
            _metric(pl_module, "train_nlvr2_accuracy").update_match(nb.argmax, nb.labels, npass.B)
            _feed_scalars(pl_module, "train", nlvr2_loss=value.detach())
    else:
        _log_split(pl_module, batch, "nlvr2", nb)
        if _em(pl_module) is not None:
            _feed_split(pl_module, "nlvr2", nb, _split_groups(batch, eng.device))
            pl_module.epoch_metrics.flush()
    return ret


def compute_nlvr2_attack(pl_module, batch):
    """objectives.py:898-1000: the clean pair (nlvr2_original_*); image view: PGDAttack_nlvr2 on the CE (compute_pgd's
    img + delta_{K-1} + delta_K per image); text view: GreedyAttack_nlvr2 on the CLEAN pair (:927); the attacked pass
    (nlvr2_attacked_*) runs on (attacked or clean images, attacked or clean text) - with both views the attacked sentence with the
    attacked images (:928-930; the image-only pass of :915-923 is overwritten there and carries no gradient, it is not run).  Both
    losses carry a backward (training_step sums every key with "loss").  The reference's train branch reads the never-set
    ret["nlvr2_attacked_labels"] (defect (a)): the labels are ret["nlvr2_labels"] here.  The batch itself is not
    modified (the reference attacks deep copies)."""
    eng = pl_module.engine
    phase = "train" if pl_module.training else "val"
    npass = Nlvr2Pass.bind(pl_module, batch, "nlvr2_clean")
    npass.clean_operands()
    v_clean, lg_clean, nb_c, _ = _nlvr2_loss(pl_module, npass, batch, "clean")
    ret = {"nlvr2_original_logits": lg_clean, "nlvr2_original_loss": v_clean, "nlvr2_labels": nb_c.labels.to(torch.int64)}
    apass = npass.twin("nlvr2_att")
    npg = eng.nlvr2_bufs(npass.B, "pgd")
    npg.labels.copy_(nb_c.labels)
    if pl_module.image_view:
        pl_module.pgd_attacker.attack_pairs(pl_module, apass, npg)            # compute_pgd (:914)
        delta = pl_module.pgd_attacker.delta_log(pl_module, apass, batch)
        pl_module.log(f"nlvr2_attacked_attack/{phase}/delta", delta)
        apass.ops = [pv.patchesT_full for pv in apass.views]                  # img + delta_{K-1} + delta_K, left by the last step
    else:
        apass.clean_operands()
    if pl_module.text_view:
        aug = compute_geometric(pl_module, copy(batch), "nlvr2_attacked")     # (:927) on the clean pair
        text_stats = dict(zip(("nlvr2_attacked_num_changes", "nlvr2_attacked_change_rate"), aug["txt_attack_stats"]))
        apass.set_text(aug["text_ids"].to(eng.device, torch.int64), aug["text_masks"].to(eng.device, torch.int64))
    v_att, lg_att, nb_a, st_a = _nlvr2_loss(pl_module, apass, batch, "att", labels_from=nb_c, ref=nb_c)
    ret["nlvr2_attacked_logits"] = lg_att
    ret["nlvr2_attacked_loss"] = v_att
    if phase == "train":
        pl_module.log("nlvr2_attacked/train/loss", v_att.detach())
        pl_module.log("nlvr2_attacked/train/accuracy", _scalar(st_a[1]) / float(npass.B))
        if _em(pl_module) is not None:
            _metric(pl_module, "train_nlvr2_attacked_accuracy").update_match(nb_a.argmax, nb_a.labels, npass.B)
            views = dict(text_stats if pl_module.text_view else {}, **({"nlvr2_attacked_delta": delta} if pl_module.image_view else {}))
            _feed_scalars(pl_module, "train", nlvr2_attacked_loss=v_att.detach(), **views)
    else:
        _log_split(pl_module, batch, "nlvr2_original", nb_c)
        _log_split(pl_module, batch, "nlvr2_attacked", nb_a, ref_nb=nb_c)
        if _em(pl_module) is not None:
            group = _split_groups(batch, eng.device)
            _feed_split(pl_module, "nlvr2_original", nb_c, group)
            if pl_module.image_view or pl_module.text_view:                  # (the wrap-up reads and resets the attacked slots under a view only)
                _feed_split(pl_module, "nlvr2_attacked", nb_a, group, ref_nb=nb_c)
            pl_module.epoch_metrics.flush()
    return ret


def compute_irtr(pl_module, batch):
    """objectives.py:1180-1223: every image against its true caption and draw_false_text false ones (true first), ONE pass of B * R
    sequences (R = 1 + draw_false_text), score = rank_output(cls_feats)[:, 0] as [B, R], cross-entropy against answer 0.  The images are
    bound once; the patch rows of image b are replicated R times on the device (the reference expands the pixels)."""
    eng = pl_module.engine
    if not eng.irtr:
        raise ValueError("compute_irtr needs a model built with loss_names['irtr'] > 0 (rank_output)")
    Fn = int(pl_module.hparams.config["draw_false_text"])
    R = Fn + 1
    if R > 64:
        raise ValueError(f"draw_false_text = {Fn}: at most 63 false texts per image (include/rmcl.h rmcl_irtr_ce)")
    dev = eng.device
    ids = torch.stack([batch["text_ids"]] + [batch[f"false_text_{i}_ids"] for i in range(Fn)], dim=1).to(dev)
    msk = torch.stack([batch["text_masks"]] + [batch[f"false_text_{i}_masks"] for i in range(Fn)], dim=1).to(dev)
    B = int(ids.shape[0])
    S = B * R
    pimg = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0], tag="irtr_img")
    owner = torch.arange(B, device=dev).repeat_interleave(R)
    pb = eng.twin(pimg, "irtr", owner=owner)
    pb.d.img_type = 0
    pb.text_ids = ids.reshape(S, -1).to(torch.int64).contiguous()
    pb.text_mask = msk.reshape(S, -1).to(torch.int64).contiguous()
    per = pimg.d.P * pimg.d.patch_k
    torch.index_select(pimg.patches32.view(B, per), 0, owner, out=pb.patches32.view(S, per))
    need_grad = torch.is_grad_enabled() and pl_module.training
    op = eng.make_operand(pb, out=pb.patchesT_full)
    eng.encoder_forward(pb, key=False, mode=L.MODE_FULL if need_grad else L.MODE_INFER, patchesT=op, cls_tail=True)
    eng.heads_forward(pb, key=False, want_q=False, wgrad=need_grad)
    scores = torch.empty(S, dtype=torch.float32, device=dev)
    eng.irtr_score(pb.cls, scores)
    stats = eng.irtr_ce(scores, B, R, 1.0)
    value = _scalar(stats[0])
    if need_grad:
        def backward(grad_out, pb=pb, op=op, scores=scores):
            g = grad_out.to(torch.float32).reshape(1).contiguous()
            dscore = torch.empty(S, dtype=torch.float32, device=dev)
            eng.irtr_ce(scores, B, R, 1.0, dscore=dscore, scale_dev=g)
            dcls = eng.irtr_backward(dscore, pb.cls, torch.empty(S, pb.d.D, dtype=torch.float32, device=dev), with_grads=True)
            eng.heads_backward(pb, None, dcls, with_grads=True)
            eng.encoder_backward(pb, L.MODE_FULL, op, pb.dcls, cls_only=True, dpatches=None)
            pl_module.after_backward()

        value = _DeferredBackward.apply(pl_module.grad_anchor, value, backward, pl_module.grad_prescale())
    phase = "train" if pl_module.training else "val"
    pl_module.log(f"irtr/{phase}/irtr_loss", value.detach())
    _feed_scalars(pl_module, phase, irtr_loss=value.detach())
    return {"irtr_loss": value, "irtr_scores": scores.view(B, R)}


# ---- IRTR recall evaluation (objectives.py:1226-1346) ---------------------------------------------------------------------------------
def irtr_rank_split(n: int, world_size: int, rank: int) -> list:
    """Indices of the images rank `rank` scores: torch.utils.data.DistributedSampler(dataset of n, shuffle=False, drop_last=False),
    INCLUDING its wrap-around padding to ceil(n / world_size) * world_size (the reference's gathered score matrix then holds
    duplicate image rows, and its recall means count them)."""
    if n < 1 or world_size < 1 or not 0 <= rank < world_size:
        raise ValueError(f"irtr_rank_split: n={n}, world_size={world_size}, rank={rank}")
    per = -(-n // world_size)
    total = per * world_size
    idx = list(range(n))
    pad = total - n
    if pad <= n:
        idx += idx[:pad]
    else:
        idx += (idx * (-(-pad // n)))[:pad]
    return idx[rank:total:world_size]


def irtr_recall_from_scores(scores: torch.Tensor, iids: torch.Tensor, tiids: torch.Tensor):
    """(ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10) of a score matrix [rows = images (iids), columns = captions (tiids = the image
    index of every caption)], exactly as objectives.py:1318-1344: top-k over rows (text retrieval) and over columns (image retrieval)."""
    iids, tiids = iids.to(scores.device).view(-1), tiids.to(scores.device).view(-1)
    if scores.dim() != 2 or tuple(scores.shape) != (iids.numel(), tiids.numel()):
        raise ValueError(f"scores must be [images, captions] = [{iids.numel()}, {tiids.numel()}] (got {tuple(scores.shape)})")
    if min(scores.shape) < 10:
        raise ValueError(f"R@10 needs at least 10 images and 10 captions (got {tuple(scores.shape)}); the reference's topk(10) fails likewise")
    match = iids.view(-1, 1) == tiids.view(1, -1)                      # [images, captions]: the caption belongs to the image
    rec = {}
    n_i, n_t = match.shape
    # hits / n divided ONCE, on the host (a device division by a constant may multiply by its rounded reciprocal): fp32 scalars with
    # the bits of the reference's CPU means
    share = lambda hits, n: torch.tensor(int(hits.sum()) / n, dtype=torch.float32)
    for k in (1, 5, 10):
        best_txt = scores.topk(k, dim=1).indices                        # per image, its k best captions
        rec[f"tr{k}"] = share(match.gather(1, best_txt).any(dim=1), n_i)
        best_img = scores.topk(k, dim=0).indices                        # per caption, its k best images
        rec[f"ir{k}"] = share(match.gather(0, best_img).any(dim=0), n_t)
    return (rec["ir1"], rec["ir5"], rec["ir10"], rec["tr1"], rec["tr5"], rec["tr10"])


def irtr_tiles(counts, n_txt: int, tile_images: int, tile_texts: int):
    """Schedule of the rank passes: images sorted by patch count (stable) and cut into groups of `tile_images`, so a tile is padded only
    to ITS OWN longest image; every group meets the captions in chunks of `tile_texts`.  Yields (image slots, padded patch count,
    first caption, end caption)."""
    order = sorted(range(len(counts)), key=lambda i: (counts[i], i))
    for g0 in range(0, len(order), tile_images):
        grp = order[g0:g0 + tile_images]
        n = max(counts[i] for i in grp)
        for t0 in range(0, n_txt, tile_texts):
            yield grp, n, t0, min(n_txt, t0 + tile_texts)


def _irtr_batches(dset, indices, batch_size, mlm_collator):
    """collated batches of dset[indices]: a dataset with the reference's protocol (__getitem__ + collate), or a sequence of batches that
    are already collated (one image per entry on the image side)"""
    if hasattr(dset, "collate"):
        for i in range(0, len(indices), batch_size):
            yield dset.collate([dset[j] for j in indices[i:i + batch_size]], mlm_collator=mlm_collator)
    else:
        for j in indices:
            yield dset[j]


@torch.no_grad()
def irtr_score_matrix(pl_module, embeds, masks, counts, text_ids, text_masks, tile_images: int, tile_texts: int) -> torch.Tensor:
    """scores [n_img, n_txt] of every cached image against every caption, tile by tile (irtr_tiles) through the cached rank pass;
    the score kernel writes straight into the matrix."""
    eng = pl_module.engine
    dev = eng.device
    n_img, n_txt = int(embeds.shape[0]), int(text_ids.shape[0])
    if n_img * n_txt >= 2 ** 31:
        raise ValueError(f"score matrix of {n_img} x {n_txt} exceeds the int32 index of the score kernel")
    scores = torch.full((n_img, n_txt), float("nan"), dtype=torch.float32, device=dev)
    flat = scores.view(-1)
    for grp, n, t0, t1 in irtr_tiles(counts, n_txt, tile_images, tile_texts):
        T = t1 - t0
        slots = torch.tensor(grp, dtype=torch.int32, device=dev)
        img_of = slots.repeat_interleave(T).contiguous()
        ids = text_ids[t0:t1].repeat(len(grp), 1)
        msk = text_masks[t0:t1].repeat(len(grp), 1)
        out_index = (img_of * n_txt + torch.arange(t0, t1, dtype=torch.int32, device=dev).repeat(len(grp))).contiguous()
        rp = eng.rank_forward(ids, msk, embeds, masks, img_of, n, cls_tail=True)
        eng.irtr_score(rp.cls, flat, out_index)
    return scores


@torch.no_grad()
def compute_irtr_recall(pl_module, text_dset=None, image_dset=None, tile_images: int = 4, tile_texts: int = 64, return_scores: bool = False):
    """objectives.py:1226-1346.  Every image of the validation split against every caption: the image side (visual_embed) runs once per
    image into a device cache, the captions are cached too, and the n_img x n_txt forward passes run as tiles of tile_images x
    tile_texts (image, caption) pairs through the cached rank pass (the reference: one image x 64 captions per pass).  Without
    arguments the datasets come from pl_module.trainer.datamodule.dms[0].make_no_false_val_dset(max_num=500) like the reference's.
    Images are split over ranks as DistributedSampler(shuffle=False) does (irtr_rank_split) and the rows gathered in rank order.
    Returns (ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10); return_scores=True appends (scores, iids, tiids)."""
    eng = pl_module.engine
    if not eng.irtr:
        raise ValueError("compute_irtr_recall needs a model built with loss_names['irtr'] > 0 (rank_output)")
    dev = eng.device
    cfg = pl_module.hparams.config
    mlm = None
    if text_dset is None or image_dset is None:
        dm = pl_module.trainer.datamodule.dms[0]
        mlm = getattr(dm, "mlm_collator", None)
        if text_dset is None:
            text_dset = dm.make_no_false_val_dset(max_num=500)
            text_dset.tokenizer = dm.tokenizer
        if image_dset is None:
            image_dset = dm.make_no_false_val_dset(image_only=True, max_num=500)
            image_dset.tokenizer = dm.tokenizer
    ids, msks, tiids = [], [], []
    for b in _irtr_batches(text_dset, list(range(len(text_dset))), 64, mlm):
        ids.append(b["text_ids"].to(dev))
        msks.append(b["text_masks"].to(dev))
        tiids += [int(i) for i in b["img_index"]]
    text_ids, text_masks = torch.cat(ids).to(torch.int64), torch.cat(msks).to(torch.int64)
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    world, rank = (torch.distributed.get_world_size(), torch.distributed.get_rank()) if dist_on else (1, 0)
    mine = irtr_rank_split(len(image_dset), world, rank)
    per_image, iids = [], []
    over = 0
    for b in _irtr_batches(image_dset, mine, 1, mlm):
        if eng.long_sequences:
            # an image past the 512-token limit cannot be embedded at all (the library's dims end there): it is only counted, so that
            # this rank reaches the reduction below and every rank raises together
            n_i = eng.patch_count(b["image"][0], cfg["max_image_len"])
            if n_i + 1 + int(cfg["max_text_len"]) > eng.token_cap:
                over = max(over, n_i)
                continue
        ie, im, _, _ = pl_module.visual_embed(b["image"][0].to(dev), max_image_len=cfg["max_image_len"], mask_it=False)
        per_image.append((ie, im))
        iids.append(int(b["img_index"][0]))
    counts = [int(ie.shape[1]) - 1 for ie, _ in per_image]
    n_max = max(counts + [over])
    if world > 1:
        # every rank sees the longest image of the WHOLE split: all of them raise below, none is left waiting in the gather
        longest = torch.tensor([n_max], dtype=torch.int64, device=dev)
        torch.distributed.all_reduce(longest, op=torch.distributed.ReduceOp.MAX)
        n_max = int(longest)
    # the token limit is checked HERE, on the whole image cache, before the first pair is scored
    if eng.dtype == L.BF16 and n_max + 1 + int(cfg["max_text_len"]) > eng.token_cap:
        raise eng.token_limit_error(n_max)
    embeds = torch.zeros(len(per_image), n_max + 1, int(cfg["hidden_size"]), dtype=torch.float32, device=dev)
    masks = torch.zeros(len(per_image), n_max + 1, dtype=torch.int32, device=dev)
    for i, (ie, im) in enumerate(per_image):
        embeds[i, : ie.shape[1]] = ie[0]
        masks[i, : im.shape[1]] = im[0].to(torch.int32)
    del per_image
    scores = irtr_score_matrix(pl_module, embeds, masks, counts, text_ids, text_masks, int(tile_images), int(tile_texts))
    iids_t = torch.tensor(iids, dtype=torch.int64, device=dev)
    if world > 1:
        torch.distributed.barrier()
        parts = [torch.empty_like(scores) for _ in range(world)]
        iparts = [torch.empty_like(iids_t) for _ in range(world)]
        torch.distributed.all_gather(parts, scores)
        torch.distributed.all_gather(iparts, iids_t)
        scores, iids_t = torch.cat(parts), torch.cat(iparts)
    tiids_t = torch.tensor(tiids, dtype=torch.int64, device=dev)
    rec = irtr_recall_from_scores(scores, iids_t, tiids_t)
    return rec + (scores, iids_t, tiids_t) if return_scores else rec
