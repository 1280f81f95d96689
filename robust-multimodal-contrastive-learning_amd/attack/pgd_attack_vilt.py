"""PGD image attack on the MoCo objective.  Mirrors attack/pgd_attack_vilt.py:7-175 of the
reference (class names, constructor keys, ``pgd_attack(pl_module, batch, k_modality)`` -> delta),
but runs K x (encoder forward, InfoNCE, data-gradient backward, L-inf-normalised ascent step,
eps-projection) as HIP kernels with no deepcopy of the encoder and no weight-gradient work.
``PGDAttack_bartlowtwins`` (sic, :178-236) is the same loop on the Barlow-Twins cross-correlation loss, ``PGDAttack_vqa``
(:418-483) on the VQA soft-target BCE."""
from __future__ import annotations

import os

import torch

from .. import _lib as L
from .._lib import lib, check
from ..task_loss import Nlvr2Pass, InfoNceLoss, BarlowLoss, VqaLoss, Nlvr2Loss


def device_image(eng, img) -> torch.Tensor:
    """A batch image (``batch["image"][v]``) as the float tensor [B,3,H,W] on the device, for the callers that need pixels: the public
    ``pgd_attack`` methods return / leave behind images, the ITM objective mixes two views."""
    if hasattr(img, "tables"):                               # decoded bytes (collate_raw_uint8): MinMaxResize on the device first
        img = eng.resize_raw(img)
    if hasattr(img, "float_image"):                          # byte batch (collate_uint8)
        img = img.to(eng.device).float_image()
    return img.to(eng.device)


class ThreatModel:
    """The configured PGD threat model of the image attack (DESIGN.md "PGD threat models"), from the config keys

        adv_norm_img          "linf" (default) | "l2"          the ball delta is projected onto
        adv_step_rule_img     "normalised" (default) | "sign"  L-inf direction: the reference's g / max|g|, or sign(g); ignored for "l2"
                                                               (whose direction is g / ||g||_2)
        adv_random_start_img  False (default) | True           delta_0 uniform in the cube / on the sphere instead of 0
        adv_pixel_box_img     None (default) | (lo, hi)        img + delta is clamped into the box after the ball
        adv_seed_img          0                                seed of the random start

    With every key at its default (``is_default``) the attackers run the reference-shaped loop exactly as before: ``Engine.pgd_step``,
    delta_0 = 0, no box, evaluated on img + delta_{K-1} + delta_K.  Under any other value every step goes through
    ``Engine.pgd_step_ball``, and the attack is evaluated on img + delta_K."""
    NORMS = {"linf": L.PGD_BALL_LINF, "l2": L.PGD_BALL_L2}
    RULES = {"normalised": L.PGD_DIR_NORMALISED, "sign": L.PGD_DIR_SIGN}

    def __init__(self, norm="linf", step_rule="normalised", random_start=False, box=None, seed=0):
        if norm not in self.NORMS:
            raise ValueError(f"adv_norm_img must be one of {sorted(self.NORMS)} (got {norm!r})")
        if step_rule not in self.RULES:
            raise ValueError(f"adv_step_rule_img must be one of {sorted(self.RULES)} (got {step_rule!r})")
        if not isinstance(random_start, (bool, int)) or random_start not in (0, 1):
            raise ValueError(f"adv_random_start_img must be a bool (got {random_start!r})")
        if box is not None:
            try:
                lo, hi = (float(v) for v in box)
            except (TypeError, ValueError):
                raise ValueError(f"adv_pixel_box_img must be None or a pair (lo, hi) (got {box!r})") from None
            if not lo < hi:
                raise ValueError(f"adv_pixel_box_img needs lo < hi (got {box!r})")
            box = (lo, hi)
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"adv_seed_img must be an int (got {seed!r})")
        self.norm, self.step_rule, self.random_start, self.box, self.seed = norm, step_rule, bool(random_start), box, seed
        self.ball = self.NORMS[norm]
        self.direction = L.PGD_DIR_L2 if norm == "l2" else self.RULES[step_rule]
        self.is_default = norm == "linf" and step_rule == "normalised" and not self.random_start and box is None

    @classmethod
    def from_config(cls, config):
        return cls(config.get("adv_norm_img", "linf"), config.get("adv_step_rule_img", "normalised"), config.get("adv_random_start_img", False),
                   config.get("adv_pixel_box_img", None), config.get("adv_seed_img", 0))

    @staticmethod
    def mix(seed: int, counter: int) -> int:
        """the 32-bit seed of one random start: `seed` with a counter (the engine's pass counter in training, the restart number in
        RobustEval) mixed in"""
        return (int(seed) * 0x9E3779B1 + int(counter) * 0x85EBCA6B + 0x7F4A7C15) & 0xFFFFFFFF

    def step_seed(self, eng) -> int:
        """Training: adv_seed_img and the engine's pass counter, so every step draws another start and a resumed run (the counter is part
        of training_state()) continues the sequence."""
        return self.mix(self.seed, eng.pass_counter)

    def first_operand(self, eng, pb, eps, seed, clean_op=None, valid=None):
        """the operand of step 0: the random start's, or the clean image's (the caller's cast of it, if it has one)"""
        if self.random_start:
            return eng.pgd_random_start(pb, eps, self.ball, seed, self.box, valid=valid)
        return clean_op if clean_op is not None else eng.make_operand(pb)


def ascent_tail(eng, pb, step, K, lr, eps, keep_prev=False, full=None, threat=None, valid=None) -> torch.Tensor:
    """The end of PGD step `step` of K on the buffers `pb` (a whole batch, a lane or a view), after its data gradient is in
    ``pb.gpatch``: the L-inf-normalised ascent step with the eps projection (``Engine.pgd_step``, :162-173), which also writes the
    operand of what runs next - cast(img + delta) into ``pb.patchesT`` for the next step's forward, after the last step the attacked
    view cast(img + delta_{K-1} + delta_K) into ``full`` (default ``pb.patchesT_full``).  ``keep_prev``: delta_{K-1} is left in
    ``pb.delta_prev``.  Returns the operand written.
    ``threat``: a non-default ``ThreatModel`` - the step is ``Engine.pgd_step_ball`` (its direction, ball and box; ``valid``: per-sample
    valid element counts), the last step writes cast(box(img + delta_K)), and delta_prev is not produced."""
    last = step == K - 1
    if threat is not None and not threat.is_default:
        op = (pb.patchesT_full if full is None else full) if last else pb.patchesT
        return eng.pgd_step_ball(pb, lr, eps, threat.direction, threat.ball, threat.box, first=step == 0 and not threat.random_start, out=op,
                                 valid=valid)
    if last and keep_prev:
        if K > 1:
            pb.delta_prev.copy_(pb.delta)
        else:
            pb.delta_prev.zero_()
    op = (pb.patchesT_full if full is None else full) if last else pb.patchesT
    eng.pgd_step(pb, lr, eps, first=step == 0, out=op, sum_prev=last)
    return op


class PGDAttack:
    """The K-step loop on one image per sample: a subclass names its loss object (``loss_of``) and how ``pgd_attack`` binds a batch."""
    bind_tag = "moco"
    fp32_twin = True          # the loop runs in Engine.pgd_bufs: the fp32 twin when the engine runs PGD in fp32 (:141)
    split_lanes = False       # two half-batch chains where Engine.lanes offers them (_attack_lanes)

    def __init__(self, config, contrastive_framework):
        self.contrastive_framework = contrastive_framework
        self.adv_steps_img = config["adv_steps_img"]
        self.adv_lr_img = config["adv_lr_img"]
        self.adv_max_norm_img = config["adv_max_norm_img"]
        self.max_image_len = config["max_image_len"]
        self.threat = ThreatModel.from_config(config)          # (unknown values: ValueError here, at construction)

    def loss_of(self, pl_module, pb, target):
        """the objective's loss object (task_loss.py) against `target`: the keys, or the buffers holding the batch's labels"""
        raise NotImplementedError(f"pgd_attack of {self.contrastive_framework} isn't implemented.")

    def bind(self, pl_module, batch, img_init, k_modality):          # -> (pass buffers, target) for the public ``pgd_attack``
        return pl_module.engine.bind_batch(batch["text_ids"], batch["text_masks"], img_init, tag=self.bind_tag), k_modality

    def pgd_attack(self, pl_module, batch, k_modality=None):
        """Returns delta_K in image layout.  Reference-shaped loop (default keys): leaves batch['image'][0] = img + delta_{K-1}, the
        reference's quirk - its callers then add delta_K on top.  Configured threat model: leaves img + delta_K, the image the returned
        delta belongs to (already inside the pixel box, if one is set)."""
        eng = pl_module.engine
        img_init = device_image(eng, batch["image"][0])
        pb, target = self.bind(pl_module, batch, img_init, k_modality)
        delta_p = self.attack_patches(pl_module, pb, target, keep_prev=self.threat.is_default)
        if not self.threat.is_default:
            delta = eng.patches_to_image(delta_p, pb)
            batch["image"][0] = img_init + delta
            return delta
        # the reference leaves batch['image'][0] = img_init + delta_{K-1} behind (:144)
        batch["image"][0] = img_init + eng.patches_to_image(pb.delta_prev, pb)
        return eng.patches_to_image(delta_p, pb)

    def attack_patches(self, pl_module, pb, target, before_first_loss=None, clean_out=None, keep_prev=False, clean_op=None, key_stream=None,
                       key_event=None):
        """K-step attack in patch layout.  Leaves delta_K in ``pb.delta`` and the ATTACKED VIEW's operand
        cast(img + delta_{K-1} + delta_K) (see compute_pgd / objectives.py:176) in ``pb.patchesT_full``; with ``keep_prev``
        also delta_{K-1} in ``pb.delta_prev`` (the public ``pgd_attack`` needs it for the batch image it leaves behind).
        ``target``: the keys - VQA: VqaBuffers holding this batch's label / score tables (Engine.vqa_targets), the loop's head runs in them.
        ``before_first_loss``: callback run once between the first encoder forward and the first InfoNCE (the
        caller joins the key-encoder stream there).  ``clean_out``: dict that receives the clean-query statistics:
        step 0 evaluates the query encoder at img + delta_0 = img, i.e. it IS the clean forward of
        objectives.py:267-275, so that forward is not computed twice when dropout is off."""
        eng = pl_module.engine
        loss = self.loss_of(pl_module, pb, target)
        pb0, pb = pb, (eng.pgd_bufs(pb) if self.fp32_twin else pb)
        seed = self.threat.step_seed(eng) if self.threat.random_start else 0    # before any pass of this attack advances the counter
        if self.threat.random_start and clean_out is not None:
            # step 0 no longer runs on the clean image: the clean-query statistics come from a forward of their own
            loss.forward(pb, clean_op if (clean_op is not None and pb is pb0) else eng.make_operand(pb), L.MODE_INFER, want_grad=False, scale=0.0,
                         wgrad=False, before_loss=before_first_loss, clean_out=clean_out)
            before_first_loss = clean_out = None
        lanes = eng.lanes(pb) if (self.split_lanes and pb is pb0) else None
        if lanes is not None:
            return self._attack_lanes(eng, pb, loss, lanes, before_first_loss, clean_out, keep_prev, clean_op, key_stream, key_event, seed)
        first = {n: v for n, v in (("before_loss", before_first_loss), ("clean_out", clean_out)) if v is not None}
        return self._attack_chain(eng, pb, loss, first, clean_op if pb is pb0 else None, keep_prev, pb0.patchesT_full, seed)

    def _attack_chain(self, eng, pb, loss, first, clean_op=None, keep_prev=False, full=None, seed=0):
        """K steps as one chain on the current stream: the loss object's forward at img + delta (encoder, pooler / projection heads,
        the objective's loss; step 0 with the hooks `first`) and its data-gradient backward, then ``ascent_tail``.  Every step's
        update kernel also writes the next forward's operand, step 0 starts from the implicit delta_0 = 0: no zero fills, no separate
        add + cast passes, no delta copy inside the loop.  ``clean_op``: the caller's cast of the clean image in pb.patchesT, if it
        has one; ``full``: where the attacked view's operand goes (``ascent_tail``).  Returns ``pb.delta`` = delta_K."""
        K = self.adv_steps_img
        op = self.threat.first_operand(eng, pb, self.adv_max_norm_img, seed, clean_op)     # img_init + delta_0; delta_0 = 0 (:136,144) by default
        for step in range(K):
            loss.forward(pb, op, L.MODE_DATA, K, wgrad=False, **(first if step == 0 else {}))
            loss.backward(pb, op, L.MODE_DATA, dpatches=pb.gpatch)
            op = ascent_tail(eng, pb, step, K, self.adv_lr_img, self.adv_max_norm_img, keep_prev, full, threat=self.threat)
        return pb.delta


class PGDAttack_moco(PGDAttack):
    split_lanes = True

    def __init__(self, config):
        super().__init__(config, "moco")

    def loss_of(self, pl_module, pb, k):
        if k is not None and k.data_ptr() != pb.k.data_ptr():
            pb.k.copy_(k)
        return InfoNceLoss(pl_module, metrics=False)          # CE(label 0) / K (:152-158); only dq and the prediction are read

    def _attack_lanes(self, eng, pb, loss, lanes, before_first_loss, clean_out, keep_prev, clean_op, key_stream, key_event=None, seed=0):
        """The same K steps as two independent half-batch chains (Engine.lanes): lane 0 on the current stream, lane 1 on
        ``eng.side_stream`` (RMCL_LANE_LAG_US: an extra start delay of lane 1; the host's call-by-call enqueue order already staggers them).
        Every per-sample buffer of a lane is a view of ``pb``'s, so ``pb`` ends up exactly as the one-chain loop leaves it.
        ``key_stream`` / ``key_event``: where the keys are produced, if not on the current stream (lane 1 waits for the event - or the
        whole stream - by itself before its first InfoNCE)."""
        K = self.adv_steps_img
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
        if self.threat.random_start:                           # every lane draws its own samples' start (sample0 = lane * B): the one-chain bits
            for i, ln in enumerate(lanes):
                with on(i):
                    ops[i] = self.threat.first_operand(eng, ln, self.adv_max_norm_img, seed)

        check(lib.rmcl_tune_set(10, len(lanes)), "tune_set")  # the GEMM routing sizes a launch against its share of the CUs
        try:
            for step in range(K):
                # the host alternates between the lanes call by call, so that neither queue runs dry while the other is being filled
                for i, ln in enumerate(lanes):
                    with on(i):
                        eng.encoder_forward(ln, key=False, mode=L.MODE_DATA, patchesT=ops[i], cls_tail=True)
                        loss.pool(ln, False)
                for i, ln in enumerate(lanes):
                    with on(i):
                        if step == 0:
                            if i == 0 and before_first_loss is not None:
                                before_first_loss()
                            if i > 0 and key_event is not None:
                                streams[i].wait_event(key_event)
                            elif i > 0 and key_stream is not None and key_stream is not streams[i]:
                                streams[i].wait_stream(key_stream)
                        loss.loss_forward(ln, ln.cls, loss.scale(pb, K), True)                      # 1 / B of the WHOLE batch (:152-158)
                        if step == 0 and clean_out is not None:
                            clean_out["prediction"][i * ln.B:(i + 1) * ln.B].copy_(ln.rows[:, 1])
                            clean_out["q"][i * ln.B:(i + 1) * ln.B].copy_(ln.q)
                        loss.head_backward(ln, False)
                for i, ln in enumerate(lanes):
                    with on(i):
                        eng.encoder_backward(ln, L.MODE_DATA, ops[i], ln.dcls, cls_only=True, dpatches=ln.gpatch)
                for i, ln in enumerate(lanes):
                    with on(i):
                        ops[i] = ascent_tail(eng, ln, step, K, self.adv_lr_img, self.adv_max_norm_img, keep_prev, threat=self.threat)
        finally:
            # process-global routing state and the forked streams are put back on EVERY path: an exception inside the loop must not
            # leave every later GEMM sized for half the chip or the side streams unjoined
            check(lib.rmcl_tune_set(10, 1), "tune_set")
            for st in streams[1:]:
                main.wait_stream(st)
        return pb.delta


class PGDAttack_bartlowtwins(PGDAttack):
    """attack/pgd_attack_vilt.py:178-236 (the reference's spelling of the class name is kept): loss =
    (on_diag + adv_lr * off_diag) / K on c = q^T k / B over the LOCAL batch, q = barlowtwins_head(cls_feats) of a deep copy of
    the head: batch statistics in training (the module's running estimates stay untouched), the running estimates in
    validation."""
    bind_tag = "bt"
    fp32_twin = False         # (this loop has always run in the batch's own buffers)

    def __init__(self, config):
        super().__init__(config, "barlowtwins")

    def loss_of(self, pl_module, pb, zk):
        return BarlowLoss(pl_module, "pgd", zk)

    def bind(self, pl_module, batch, img_init, k_modality):
        pb, _ = super().bind(pl_module, batch, img_init, None)
        return pb, k_modality.to(pl_module.engine.device, torch.float32).contiguous()


class PGDAttack_vqa(PGDAttack):
    """attack/pgd_attack_vilt.py:418-483: K steps of (forward at img + delta, vqa_classifier, BCE-with-logits x vqav2_label_size - NOT
    divided by K, data gradient, L-inf-normalised ascent step with the 1e-8 clamp, clip to eps).  The reference runs the live
    module and its backward() also leaves weight gradients in .grad; under its fp16 recipe those are removed by the loss scale
    (INTEGRATION.md), so here the loop runs data gradients only: encoder MODE_DATA, head backward without weight gradients -
    nothing is written into the gradient arena."""
    bind_tag = "vqa_att"

    def __init__(self, config):
        super().__init__(config, "vqa")

    def loss_of(self, pl_module, pb, vb_tables):
        return VqaLoss(pl_module, vb_tables)                    # :444-460 ... :464-481

    def bind(self, pl_module, batch, img_init, k_modality):
        pb, eng = super().bind(pl_module, batch, img_init, None)[0], pl_module.engine
        return pb, eng.vqa_targets(eng.vqa_bufs(pb.B, "pgd"), batch["vqa_labels"], batch["vqa_scores"])


def pair_valid(eng, pv, pair, attack_idx):
    """Valid element counts of a view's samples with the images that are not attacked (attack_idx) set to 0: such a sample is all pad
    slots to the threat-model kernels - delta stays 0 and its operand is the clean image.  None: every element of every sample."""
    a0, a1 = attack_idx
    valid = eng.pgd_valid(pv)
    if not pair or (a0 and a1):
        return valid
    valid = torch.full((pv.B,), pv.d.P * pv.d.patch_k, dtype=torch.int32, device=eng.device) if valid is None else valid.clone()
    valid.view(-1, 2)[:, 1 if a0 else 0] = 0
    return valid


def pair_images(eng, npass, pats, shapes):
    """(image_0 part, image_1 part) of per-view patch tensors `pats` (one per view of `npass`), in the batch's image layouts `shapes`"""
    if npass.pair:
        img = eng.patches_to_image(pats[0], npass.views[0])
        return tuple(img[k::2, :, : shapes[k][2], : shapes[k][3]] for k in range(2))
    return tuple(eng.patches_to_image(pat, pv) for pat, pv in zip(pats, npass.views))


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
        K, loss = self.adv_steps_img, Nlvr2Loss(pl_module, nb)
        a0, a1 = self.attack_idx[0], self.attack_idx[1]
        views = npass.views
        if npass.pair:
            attacked = [a0 or a1]
        else:
            attacked = [a0, a1]
        if not self.threat.is_default:
            return self._attack_pairs_threat(eng, npass, loss, attacked)
        npass.clean_operands(full_buffer=False)                             # img + delta_0, delta_0 = 0 (:266-271)
        for i, pv in enumerate(views):
            if not attacked[i]:                                             # never stepped: delta 0, the attacked view is the clean one
                pv.delta.zero_()
                pv.delta_prev.zero_()
                eng.make_operand(pv, out=pv.patchesT_full)
        for step in range(K):
            loss.forward(npass, None, L.MODE_DATA, K, wgrad=False)                            # CE / adv_steps_img (:296)
            loss.backward(npass, None, L.MODE_DATA, dpatches=attacked)
            for i, pv in enumerate(views):
                if not attacked[i]:
                    continue
                if npass.pair and not (a0 and a1):                          # the image that is not attacked: zero gradient rows -> step 0
                    pv.gpatch.view(npass.B, 2, -1)[:, 1 if a0 else 0].zero_()
                npass.ops[i] = ascent_tail(eng, pv, step, K, self.adv_lr_img, self.adv_max_norm_img, keep_prev)   # :302-331

    def _attack_pairs_threat(self, eng, npass, loss, attacked):
        """attack_pairs under a configured threat model: optional random start, K x (forward, data gradient, pgd_step_ball); the last
        step leaves cast(box(img + delta_K)) in ``pv.patchesT_full``.  One seed for all views: sample b of both images draws from its
        own index (pair form: rows 2b, 2b + 1; two-pass form: the views use seed and seed + 1)."""
        K, th, seed = self.adv_steps_img, self.threat, self.threat.step_seed(eng)
        valids = [pair_valid(eng, pv, npass.pair, self.attack_idx) for pv in npass.views]
        npass.ops = [None] * len(npass.views)
        for i, pv in enumerate(npass.views):
            if attacked[i]:
                npass.ops[i] = th.first_operand(eng, pv, self.adv_max_norm_img, (seed + i) & 0xFFFFFFFF, valid=valids[i])
            else:                                                           # never stepped: delta 0, the attacked view is the clean one
                pv.delta.zero_()
                npass.ops[i] = eng.make_operand(pv, out=pv.patchesT_full)
        for step in range(K):
            loss.forward(npass, None, L.MODE_DATA, K, wgrad=False)
            loss.backward(npass, None, L.MODE_DATA, dpatches=attacked)
            for i, pv in enumerate(npass.views):
                if attacked[i]:
                    npass.ops[i] = ascent_tail(eng, pv, step, K, self.adv_lr_img, self.adv_max_norm_img, threat=th, valid=valids[i])

    def _image_of(self, eng, npass, pat_attr, shapes):
        """(image_0 part, image_1 part) of a per-view patch buffer, in the batch's image layouts"""
        return pair_images(eng, npass, [getattr(pv, pat_attr) for pv in npass.views], shapes)

    def delta_log(self, pl_module, npass, batch):
        """(mean_c ||delta_0||_c + mean_c ||delta_1||_c) / sum(attack_idx) (objectives.py:179-184), from the patch-layout deltas."""
        eng = pl_module.engine
        n_att = sum(self.attack_idx)
        shapes = [tuple(batch["image_0"][0].shape), tuple(batch["image_1"][0].shape)]
        if npass.pair and shapes[0] != shapes[1]:                            # two padded extents: per-image means of the image tensors
            d0, d1 = self._image_of(eng, npass, "delta", shapes)
            return (torch.linalg.norm(d0, dim=1).mean() + torch.linalg.norm(d1, dim=1).mean()) / n_att
        out = torch.zeros(len(npass.views), dtype=torch.float32, device=eng.device)
        for i, pv in enumerate(npass.views):                                 # (pair form: one sum over both images of the same extent)
            eng.delta_channel_norm(pv, out[i:i + 1])
        n_pix = [float(npass.B * sh[2] * sh[3]) for sh in shapes]           # every image of a key: B x H x W pixels
        return ((out[0] / n_pix[0] if npass.pair else out[0] / n_pix[0] + out[1] / n_pix[1]) / n_att).reshape(())

    def pgd_attack(self, pl_module, batch, k_modality=None):
        """The reference's public form: returns (delta_0, delta_1) in image layout and leaves image_k = img_k + delta_{K-1} in the batch."""
        eng = pl_module.engine
        imgs = []
        for key in ("image_0", "image_1"):
            imgs.append(device_image(eng, batch[key][0]).to(torch.float32))
        b2 = dict(batch, image_0=[imgs[0]], image_1=[imgs[1]])
        npass = Nlvr2Pass.bind(pl_module, b2, "nlvr2_att_0").twin("nlvr2_att")
        nb = eng.nlvr2_bufs(npass.B, "pgd")
        eng.nlvr2_labels(nb, batch["answers"])
        self.attack_pairs(pl_module, npass, nb, keep_prev=self.threat.is_default)
        shapes = [tuple(i.shape) for i in imgs]
        deltas = self._image_of(eng, npass, "delta", shapes)
        # configured threat model: img_k + delta_K, the images the returned deltas belong to (PGDAttack.pgd_attack)
        prevs = self._image_of(eng, npass, "delta_prev", shapes) if self.threat.is_default else deltas
        batch["image_0"][0] = imgs[0] + prevs[0]
        batch["image_1"][0] = imgs[1] + prevs[1]
        return deltas[0].contiguous(), deltas[1].contiguous()
