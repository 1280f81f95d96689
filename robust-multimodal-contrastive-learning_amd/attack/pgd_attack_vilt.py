"""PGD image attack on the MoCo objective.  Mirrors attack/pgd_attack_vilt.py:7-175 of the
reference (class names, constructor keys, ``pgd_attack(pl_module, batch, k_modality)`` -> delta),
but runs K x (encoder forward, InfoNCE, data-gradient backward, L-inf-normalised ascent step,
eps-projection) as HIP kernels with no deepcopy of the encoder and no weight-gradient work.
``PGDAttack_bartlowtwins`` (sic, :178-236) is the same loop on the Barlow-Twins cross-correlation loss, ``PGDAttack_vqa``
(:418-483) on the VQA soft-target BCE."""
from __future__ import annotations

import torch

from .. import _lib as L


def device_image(eng, img) -> torch.Tensor:
    """A batch image (``batch["image"][v]``) as the float tensor [B,3,H,W] on the device, for the callers that need pixels: the public
    ``pgd_attack`` methods return / leave behind images, the ITM objective mixes two views."""
    if hasattr(img, "tables"):                               # decoded bytes (collate_raw_uint8): MinMaxResize on the device first
        img = eng.resize_raw(img)
    if hasattr(img, "float_image"):                          # byte batch (collate_uint8)
        img = img.to(eng.device).float_image()
    return img.to(eng.device)


def ascent_tail(eng, pb, step, K, lr, eps, keep_prev=False, full=None) -> torch.Tensor:
    """The end of PGD step `step` of K on the buffers `pb` (a whole batch, a lane or a view), after its data gradient is in
    ``pb.gpatch``: the L-inf-normalised ascent step with the eps projection (``Engine.pgd_step``, :162-173), which also writes the
    operand of what runs next - cast(img + delta) into ``pb.patchesT`` for the next step's forward, after the last step the attacked
    view cast(img + delta_{K-1} + delta_K) into ``full`` (default ``pb.patchesT_full``).  ``keep_prev``: delta_{K-1} is left in
    ``pb.delta_prev``.  Returns the operand written."""
    last = step == K - 1
    if last and keep_prev:
        if K > 1:
            pb.delta_prev.copy_(pb.delta)
        else:
            pb.delta_prev.zero_()
    op = (pb.patchesT_full if full is None else full) if last else pb.patchesT
    eng.pgd_step(pb, lr, eps, first=step == 0, out=op, sum_prev=last)
    return op


class PGDAttack:
    def __init__(self, config, contrastive_framework):
        self.contrastive_framework = contrastive_framework
        self.adv_steps_img = config["adv_steps_img"]
        self.adv_lr_img = config["adv_lr_img"]
        self.adv_max_norm_img = config["adv_max_norm_img"]
        self.max_image_len = config["max_image_len"]

    def pgd_attack(self, pl_module, batch, k_image):
        raise NotImplementedError(f"pgd_attack of {self.contrastive_framework} isn't implemented.")

    def _attack_chain(self, eng, pb, cls_grad, clean_op=None, keep_prev=False, full=None):
        """K steps as one chain on the current stream: encoder forward at img + delta, ``cls_grad(step)`` (the pooler / projection
        heads, the objective's loss and its head backward: returns (dq, dcls_extra), the gradient at the projection and at the pooled
        cls rows, for ``Engine.heads_backward``), data-gradient backward, ``ascent_tail``.  Every step's update kernel also writes
        the next forward's operand, step 0 starts from the implicit delta_0 = 0: no zero fills, no separate add + cast passes, no
        delta copy inside the loop.  ``clean_op``: the caller's cast of the clean image in pb.patchesT, if it has one; ``full``: where
        the attacked view's operand goes (``ascent_tail``).  Returns ``pb.delta`` = delta_K."""
        K = self.adv_steps_img
        op = clean_op if clean_op is not None else eng.make_operand(pb)     # img_init + delta_0, delta_0 = 0 (:136,144)
        for step in range(K):
            eng.encoder_forward(pb, key=False, mode=L.MODE_DATA, patchesT=op, cls_tail=True)
            dq, dcls_extra = cls_grad(step)
            eng.heads_backward(pb, dq, dcls_extra, with_grads=False)
            eng.encoder_backward(pb, L.MODE_DATA, op, pb.dcls, cls_only=True, dpatches=pb.gpatch)
            op = ascent_tail(eng, pb, step, K, self.adv_lr_img, self.adv_max_norm_img, keep_prev, full)
        return pb.delta


class PGDAttack_moco(PGDAttack):
    def __init__(self, config):
        super().__init__(config, "moco")

    def attack_patches(self, pl_module, pb, k, before_first_loss=None, clean_out=None, keep_prev=False, clean_op=None, key_stream=None, key_event=None):
        """K-step attack in patch layout.  Leaves delta_K in ``pb.delta`` and the ATTACKED VIEW's operand
        cast(img + delta_{K-1} + delta_K) (see compute_pgd / objectives.py:176) in ``pb.patchesT_full``; with ``keep_prev``
        also delta_{K-1} in ``pb.delta_prev`` (the public ``pgd_attack`` needs it for the batch image it leaves behind).

        ``before_first_loss``: callback run once between the first encoder forward and the first InfoNCE (the
        caller joins the key-encoder stream there).  ``clean_out``: dict that receives the clean-query statistics:
        step 0 evaluates the query encoder at img + delta_0 = img, i.e. it IS the clean forward of
        objectives.py:267-275, so that forward is not computed twice when dropout is off."""
        eng = pl_module.engine
        K = self.adv_steps_img
        if k is not None and k.data_ptr() != pb.k.data_ptr():
            pb.k.copy_(k)
        pb0 = pb
        pb = eng.pgd_bufs(pb)                                 # fp32 twin when the engine runs PGD in fp32 (:141)
        lanes = eng.lanes(pb) if pb is pb0 else None
        if lanes is not None:
            return self._attack_lanes(eng, pb, lanes, K, before_first_loss, clean_out, keep_prev, clean_op, key_stream, key_event)

        def cls_grad(step):
            eng.heads_forward(pb, key=False, wgrad=False)
            if step == 0 and before_first_loss is not None:
                before_first_loss()
            # CE(label 0) / K, mean over the batch (:152-158); gradient wrt q only
            eng.infonce(pb, grad_scale=1.0 / (pb.B * K), want_dq=True, metrics=False)     # (only dq and the prediction are read)
            if step == 0 and clean_out is not None:
                clean_out["prediction"] = pb.rows[:, 1].clone()
                clean_out["q"] = pb.q.clone()
            return pb.dq, None

        return self._attack_chain(eng, pb, cls_grad, clean_op if pb is pb0 else None, keep_prev, pb0.patchesT_full)

    def _attack_lanes(self, eng, pb, lanes, K, before_first_loss, clean_out, keep_prev, clean_op, key_stream, key_event=None):
        """The same K steps as two independent half-batch chains (Engine.lanes): lane 0 on the current stream, lane 1 on
        ``eng.side_stream`` (RMCL_LANE_LAG_US: an extra start delay of lane 1; the host's call-by-call enqueue order already staggers them).
        Every per-sample buffer of a lane is a view of ``pb``'s, so ``pb`` ends up exactly as the one-chain loop leaves it.
        ``key_stream`` / ``key_event``: where the keys are produced, if not on the current stream (lane 1 waits for the event - or the
        whole stream - by itself before its first InfoNCE)."""
        import os
        from .._lib import lib, check
        main = torch.cuda.current_stream()
        # lane 1 runs on the engine's side stream, BEHIND the key-encoder forward the caller may have put there: HIP multiplexes its
        # streams onto four hardware queues, and a fifth stream of this process shared the main stream's queue - the lanes then ran
        # one after the other (measured: no change of the step at all)
        side = eng.side_stream
        streams = [main, side, eng.comm_stream, eng.dw_stream][:len(lanes)]     # (four lanes: experiment, RMCL_LANE_COUNT=4)
        op_full = clean_op if clean_op is not None else eng.make_operand(pb)
        eng.fold_of(False)                                    # parameter-derived operands are refreshed on the main stream BEFORE the fork
        eng.weights_T()
        if clean_out is not None:
            clean_out["prediction"] = torch.empty(pb.B, dtype=torch.float32, device=eng.device)
            clean_out["q"] = torch.empty_like(pb.q)
        for st in streams[1:]:                                # every lane stream forks AFTER the operand / fold / transposed-weight refresh
            st.wait_stream(main)
        lag = float(os.environ.get("RMCL_LANE_LAG_US", "0"))
        if lag > 0:
            with torch.cuda.stream(side):
                torch.cuda._sleep(int(lag * 2400))            # (device spin clock: 2.4 cycles per ns on MI355X)
        per = lanes[0].B * pb.d.P
        ops = [op_full[i * per:(i + 1) * per] for i in range(len(lanes))]
        def on(i):
            return torch.cuda.stream(streams[i])

        check(lib.rmcl_tune_set(10, len(lanes)), "tune_set")  # the GEMM routing sizes a launch against its share of the CUs
        try:
            for step in range(K):
                # the host alternates between the lanes call by call, so that neither queue runs dry while the other is being filled
                for i, ln in enumerate(lanes):
                    with on(i):
                        eng.encoder_forward(ln, key=False, mode=L.MODE_DATA, patchesT=ops[i], cls_tail=True)
                        eng.heads_forward(ln, key=False, wgrad=False)
                for i, ln in enumerate(lanes):
                    with on(i):
                        if step == 0:
                            if i == 0 and before_first_loss is not None:
                                before_first_loss()
                            if i > 0 and key_event is not None:
                                streams[i].wait_event(key_event)
                            elif i > 0 and key_stream is not None and key_stream is not streams[i]:
                                streams[i].wait_stream(key_stream)
                        eng.infonce(ln, grad_scale=1.0 / (pb.B * K), want_dq=True, metrics=False)       # 1 / B of the WHOLE batch (:152-158)
                        if step == 0 and clean_out is not None:
                            clean_out["prediction"][i * ln.B:(i + 1) * ln.B].copy_(ln.rows[:, 1])
                            clean_out["q"][i * ln.B:(i + 1) * ln.B].copy_(ln.q)
                        eng.heads_backward(ln, ln.dq, None, with_grads=False)
                for i, ln in enumerate(lanes):
                    with on(i):
                        eng.encoder_backward(ln, L.MODE_DATA, ops[i], ln.dcls, cls_only=True, dpatches=ln.gpatch)
                for i, ln in enumerate(lanes):
                    with on(i):
                        ops[i] = ascent_tail(eng, ln, step, K, self.adv_lr_img, self.adv_max_norm_img, keep_prev)
        finally:
            # process-global routing state and the forked streams are put back on EVERY path: an exception inside the loop must not
            # leave every later GEMM sized for half the chip or the side streams unjoined
            check(lib.rmcl_tune_set(10, 1), "tune_set")
            for st in streams[1:]:
                main.wait_stream(st)
        return pb.delta

    def pgd_attack(self, pl_module, batch, k_modality=None):
        eng = pl_module.engine
        img_init = device_image(eng, batch["image"][0])
        pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], img_init)
        delta_p = self.attack_patches(pl_module, pb, k_modality, keep_prev=True)
        # the reference leaves batch['image'][0] = img_init + delta_{K-1} behind (:144)
        batch["image"][0] = img_init + eng.patches_to_image(pb.delta_prev, pb)
        return eng.patches_to_image(delta_p, pb)


class PGDAttack_bartlowtwins(PGDAttack):
    """attack/pgd_attack_vilt.py:178-236 (the reference's spelling of the class name is kept): loss =
    (on_diag + adv_lr * off_diag) / K on c = q^T k / B over the LOCAL batch, q = barlowtwins_head(cls_feats) of a deep copy of
    the head: batch statistics in training (the module's running estimates stay untouched), the running estimates in
    validation."""

    def __init__(self, config):
        super().__init__(config, "barlowtwins")

    def attack_patches(self, pl_module, pb, zk, keep_prev=False, clean_op=None):
        eng = pl_module.engine
        K = self.adv_steps_img
        bb = eng.bt_bufs(pb.B, "pgd")
        mode = bool(pl_module.training)           # deepcopy(pl_module.barlowtwins_head) keeps the train / eval flag (:189)

        def cls_grad(step):
            eng.heads_forward(pb, key=False, want_q=False, wgrad=False)
            eng.bt_forward(bb, pb.cls, training=mode, track=False)
            eng.bt_loss(bb, zk, float(pb.B), pl_module.adv_lr, 1.0 / K, want_dz=True)
            return None, eng.bt_backward(bb, bb.dz, training=mode, with_grads=False)

        return self._attack_chain(eng, pb, cls_grad, clean_op, keep_prev)

    def pgd_attack(self, pl_module, batch, k_modality=None):
        eng = pl_module.engine
        img_init = device_image(eng, batch["image"][0])
        pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], img_init, tag="bt")
        delta_p = self.attack_patches(pl_module, pb, k_modality.to(eng.device, torch.float32).contiguous(), keep_prev=True)
        batch["image"][0] = img_init + eng.patches_to_image(pb.delta_prev, pb)
        return eng.patches_to_image(delta_p, pb)


class PGDAttack_vqa(PGDAttack):
    """attack/pgd_attack_vilt.py:418-483: K steps of (forward at img + delta, vqa_classifier, BCE-with-logits x vqav2_label_size - NOT
    divided by K, data gradient, L-inf-normalised ascent step with the 1e-8 clamp, clip to eps).  The reference runs the live
    module and its backward() also leaves weight gradients in .grad; under its fp16 recipe those are removed by the loss scale
    (INTEGRATION.md), so here the loop runs data gradients only: encoder MODE_DATA, head backward without weight gradients -
    nothing is written into the gradient arena."""

    def __init__(self, config):
        super().__init__(config, "vqa")

    def attack_patches(self, pl_module, pb, vb_tables, clean_op=None, keep_prev=False):
        """Leaves delta_K in ``pb.delta`` and the attacked view's operand cast(img + delta_{K-1} + delta_K) (compute_pgd,
        objectives.py:176) in ``pb.patchesT_full``.  ``vb_tables``: VqaBuffers holding this batch's label / score tables
        (Engine.vqa_targets); the loop's head passes run in them."""
        eng = pl_module.engine
        pb0 = pb
        pb = eng.pgd_bufs(pb)                                 # fp32 twin when the engine runs PGD in fp32
        vb = vb_tables

        def cls_grad(step):
            eng.heads_forward(pb, key=False, want_q=False, wgrad=False)
            eng.vqa_forward(vb, pb.cls)
            eng.vqa_bce(vb, 1.0, want_dz=True)                                        # :444-460, d loss / d logits
            return None, eng.vqa_backward(vb, vb.dz, with_grads=False)

        return self._attack_chain(eng, pb, cls_grad, clean_op if pb is pb0 else None, keep_prev, pb0.patchesT_full)   # :464-481

    def pgd_attack(self, pl_module, batch, k_modality=None):
        eng = pl_module.engine
        img_init = device_image(eng, batch["image"][0])
        pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], img_init, tag="vqa_att")
        vb = eng.vqa_targets(eng.vqa_bufs(pb.B, "pgd"), batch["vqa_labels"], batch["vqa_scores"])
        delta_p = self.attack_patches(pl_module, pb, vb, keep_prev=True)
        batch["image"][0] = img_init + eng.patches_to_image(pb.delta_prev, pb)
        return eng.patches_to_image(delta_p, pb)


class PGDAttack_nlvr2(PGDAttack):
    """attack/pgd_attack_vilt.py:241-342: K steps on the pair (image_0 with token type 1, image_1 with token type 2), loss =
    CE(nlvr2_classifier(cat(cls_0, cls_1)), answers) / K, one delta per image, updated only where config["attack_idx"][i] is set (a
    non-attacked image keeps delta 0), each step the L-inf-normalised ascent step with the 1e-8 clamp and the clip to eps.  The reference
    runs a deep copy of the modules, so nothing reaches the live model's gradients: here the loop runs data gradients only (encoder
    MODE_DATA, head backward without weight gradients) and writes nothing into the gradient arena.  In the pair form both deltas live
    in one patch-layout buffer of 2B samples: pgd_step's per-sample step is per image."""

    def __init__(self, config):
        super().__init__(config, "nlvr2")
        self.attack_idx = [bool(a) for a in config["attack_idx"]]

    def attack_pairs(self, pl_module, npass, nb, keep_prev=False):
        """Leaves delta_K of every view in ``pv.delta`` and the attacked operand cast(img + delta_{K-1} + delta_K) (compute_pgd,
        objectives.py:166-174) in ``pv.patchesT_full``; with ``keep_prev`` also delta_{K-1} in ``pv.delta_prev``.  ``nb``: Nlvr2Buffers
        holding the batch's labels; the loop's head passes run in them."""
        eng = pl_module.engine
        K = self.adv_steps_img
        a0, a1 = self.attack_idx[0], self.attack_idx[1]
        views = npass.views
        if npass.pair:
            attacked = [a0 or a1]
        else:
            attacked = [a0, a1]
        npass.clean_operands(full_buffer=False)                             # img + delta_0, delta_0 = 0 (:266-271)
        for i, pv in enumerate(views):
            if not attacked[i]:                                             # never stepped: delta 0, the attacked view is the clean one
                pv.delta.zero_()
                pv.delta_prev.zero_()
                eng.make_operand(pv, out=pv.patchesT_full)
        for step in range(K):
            cls2 = npass.forward(L.MODE_DATA, wgrad=False)
            eng.nlvr2_forward(nb, cls2)
            eng.nlvr2_ce(nb, 1.0 / K, want_dz=True)                          # CE / adv_steps_img (:296)
            dcls2 = eng.nlvr2_backward(nb, nb.dz, with_grads=False)
            npass.backward(dcls2, L.MODE_DATA, with_grads=False, dpatches=attacked)
            for i, pv in enumerate(views):
                if not attacked[i]:
                    continue
                if npass.pair and not (a0 and a1):                          # the image that is not attacked: zero gradient rows -> step 0
                    pv.gpatch.view(npass.B, 2, -1)[:, 1 if a0 else 0].zero_()
                npass.ops[i] = ascent_tail(eng, pv, step, K, self.adv_lr_img, self.adv_max_norm_img, keep_prev)   # :302-331

    def _image_of(self, eng, npass, pat_attr, shapes):
        """(image_0 part, image_1 part) of a per-view patch buffer, in the batch's image layouts"""
        if npass.pair:
            pv = npass.views[0]
            img = eng.patches_to_image(getattr(pv, pat_attr), pv)
            return tuple(img[k::2, :, : shapes[k][2], : shapes[k][3]] for k in range(2))
        return tuple(eng.patches_to_image(getattr(pv, pat_attr), pv) for pv in npass.views)

    def delta_log(self, pl_module, npass, batch):
        """(mean_c ||delta_0||_c + mean_c ||delta_1||_c) / sum(attack_idx) (objectives.py:179-184), from the patch-layout deltas."""
        from .._lib import lib, check, P, I64
        from ..runtime import stream_ptr
        eng = pl_module.engine
        n_att = sum(self.attack_idx)
        shapes = [tuple(batch["image_0"][0].shape), tuple(batch["image_1"][0].shape)]
        if npass.pair and shapes[0] != shapes[1]:                            # two padded extents: per-image means of the image tensors
            d0, d1 = self._image_of(eng, npass, "delta", shapes)
            return (torch.linalg.norm(d0, dim=1).mean() + torch.linalg.norm(d1, dim=1).mean()) / n_att
        out = torch.zeros(len(npass.views), dtype=torch.float32, device=eng.device)
        for i, pv in enumerate(npass.views):                                 # (pair form: one sum over both images of the same extent)
            check(lib.rmcl_delta_channel_norm(P(pv.delta), P(out[i:i + 1]), I64(pv.delta.shape[0]), 3, pv.d.patch_k // 3, stream_ptr()),
                  "delta_norm")
        n_pix = [float(npass.B * sh[2] * sh[3]) for sh in shapes]           # every image of a key: B x H x W pixels
        return ((out[0] / n_pix[0] if npass.pair else out[0] / n_pix[0] + out[1] / n_pix[1]) / n_att).reshape(())

    def pgd_attack(self, pl_module, batch, k_modality=None):
        """The reference's public form: returns (delta_0, delta_1) in image layout and leaves image_k = img_k + delta_{K-1} in the batch."""
        from ..vilt.modules.objectives import Nlvr2Pass
        eng = pl_module.engine
        imgs = []
        for key in ("image_0", "image_1"):
            imgs.append(device_image(eng, batch[key][0]).to(torch.float32))
        b2 = dict(batch, image_0=[imgs[0]], image_1=[imgs[1]])
        npass = Nlvr2Pass.bind(pl_module, b2, "nlvr2_att_0").twin("nlvr2_att")
        nb = eng.nlvr2_bufs(npass.B, "pgd")
        eng.nlvr2_labels(nb, batch["answers"])
        self.attack_pairs(pl_module, npass, nb, keep_prev=True)
        shapes = [tuple(i.shape) for i in imgs]
        deltas = self._image_of(eng, npass, "delta", shapes)
        prevs = self._image_of(eng, npass, "delta_prev", shapes)
        batch["image_0"][0] = imgs[0] + prevs[0]
        batch["image_1"][0] = imgs[1] + prevs[1]
        return deltas[0].contiguous(), deltas[1].contiguous()
