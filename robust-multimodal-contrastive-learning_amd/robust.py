"""Robustness evaluation of a fine-tuned VQA or NLVR2 model: ``RobustEval(model).attack`` runs PGD on the image(s) of a batch under a
configured threat model - L-inf or L2 ball, sign / normalised / L2 step, random start, pixel box, restarts - and ``curve`` turns a
stream of batches into score-versus-eps numbers.  DESIGN.md "PGD threat models", INTEGRATION.md "Robustness evaluation".

Everything runs on the passes the training path already has: the task's loss object (task_loss.py), data-gradient backwards only
(``MODE_DATA``: nothing is written to the gradient arena), and the three kernels of csrc/pgd_ball.hip - ``Engine.pgd_random_start``,
``Engine.pgd_step_ball``, ``Engine.pgd_keep_worst``.  The worst restart of every sample is chosen on the device from the per-sample loss
the task's loss kernel writes; no result is read back.  The attack is evaluated on img + delta_K (not on the reference loop's
img + delta_{K-1} + delta_K).  There is no text attack here.

A call borrows the model as ``Predictor`` does: eval mode, dropout off, and the mode flags, the dropout switch and the engine's pass
counter are put back afterwards, so a training step taken after an evaluation has the loss bits it would have had without it."""
from __future__ import annotations

import contextlib

import torch

from . import _lib as L
from .attack.pgd_attack_vilt import ThreatModel, device_image, pair_images, pair_valid
from .task_loss import Nlvr2Pass, VqaLoss, Nlvr2Loss


class _Bound:
    """One bound batch: the task's view and loss object, the per-view perturbation buffers, and the clean results."""


class RobustEval:
    """``RobustEval(model)``: the task is read from the model - ``engine.vqa`` (loss_names["vqa"] / ["vqa_attacked"]) or ``engine.nlvr2``."""

    def __init__(self, model):
        self.model, self.eng = model, model.engine
        if self.eng.vqa is not None:
            self.task = "vqa"
        elif self.eng.nlvr2 is not None:
            self.task = "nlvr2"
        else:
            raise ValueError("RobustEval needs a model with the VQA head (loss_names['vqa'] or ['vqa_attacked'] > 0) or the NLVR2 head "
                             "(loss_names['nlvr2'] or ['nlvr2_attacked'] > 0); this model has neither")

    @contextlib.contextmanager
    def _eval(self):
        eng = self.eng
        flags = [(m, m.training) for m in self.model.modules()]
        saved = (eng.dropout_on, eng.pass_counter)
        self.model.eval()
        eng.dropout_on = False
        try:
            with torch.no_grad():
                yield
        finally:
            for m, t in flags:
                m.training = t
            eng.dropout_on, eng.pass_counter = saved

    # ---- binding and the clean forward ---------------------------------------------------------------------------------------
    def _bind(self, batch) -> _Bound:
        eng, b = self.eng, _Bound()
        if self.task == "vqa":
            pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0], tag="robust")
            vb = eng.vqa_targets(eng.vqa_bufs(pb.B, "robust"), batch["vqa_labels"], batch["vqa_scores"])
            b.view, b.views, b.pair, b.B, b.head, b.loss = pb, [pb], False, pb.B, vb, VqaLoss(self.model, vb)
            b.attacked, b.valids = [True], [None]
        else:
            imgs = [device_image(eng, batch[k][0]).to(torch.float32) for k in ("image_0", "image_1")]
            npass = Nlvr2Pass.bind(self.model, dict(batch, image_0=[imgs[0]], image_1=[imgs[1]]), "robust")
            nb = eng.nlvr2_bufs(npass.B, "robust")
            eng.nlvr2_labels(nb, batch["answers"])
            b.view, b.views, b.pair, b.B, b.head, b.loss = npass, npass.views, npass.pair, npass.B, nb, Nlvr2Loss(self.model, nb)
            b.shapes = [tuple(i.shape) for i in imgs]
            idx = [bool(a) for a in self.model.hparams.config.get("attack_idx", [True, True])]
            b.attacked = [idx[0] or idx[1]] if npass.pair else idx
            b.valids = [pair_valid(eng, pv, npass.pair, idx) for pv in npass.views]
        b.rows_per_decision = 2 if b.pair else 1
        b.best_delta = [torch.zeros_like(pv.delta) for pv in b.views]
        b.best_op = [torch.empty_like(pv.patchesT_full) for pv in b.views]
        b.best_score = [torch.empty(b.B, dtype=torch.float32, device=eng.device) for _ in b.views]
        b.best_restart = [torch.zeros(b.B, dtype=torch.int32, device=eng.device) for _ in b.views]
        b.clean_ops = [eng.make_operand(pv, out=torch.empty_like(pv.patchesT_full)) for pv in b.views]
        b.clean = self._results(b, b.clean_ops)
        return b

    def _set_ops(self, b, ops):
        if self.task == "nlvr2":
            b.view.ops = list(ops)

    def _forward(self, b, ops, mode, want_grad):
        self._set_ops(b, ops)
        b.loss.forward(b.view, ops[0], mode, 1, want_grad=want_grad, wgrad=False)      # the task's own loss, not divided by K

    def _results(self, b, ops):
        """one MODE_INFER forward on `ops`: (per-sample loss, prediction, per-sample score) as fresh tensors"""
        self._forward(b, ops, L.MODE_INFER, False)
        h = b.head
        if self.task == "vqa":
            return h.rows[:, 0].clone(), h.argmax.clone(), h.rows[:, 1].clone()        # rows[:, 1]: the soft target at the first maximum
        return h.rows.clone(), h.argmax.clone(), (h.argmax == h.labels).to(torch.float32)

    def _loss_column(self, b):
        return b.head.rows[:, 0] if self.task == "vqa" else b.head.rows

    # ---- the attack ----------------------------------------------------------------------------------------------------------
    def _attack_bound(self, b, eps, th: ThreatModel, steps, step_size, restarts, seed):
        eng = self.eng
        eps = float(eps)
        if not eps > 0.0 or steps < 1:                                      # the empty threat model: delta = 0, the clean results
            for bd, bo, br, op in zip(b.best_delta, b.best_op, b.best_restart, b.clean_ops):
                bd.zero_()
                bo.copy_(op)
                br.zero_()
            return b.clean
        lr = 2.5 * eps / steps if step_size is None else float(step_size)
        for r in range(restarts):
            s = ThreatModel.mix(seed, r)
            ops = []
            for i, pv in enumerate(b.views):
                if b.attacked[i] and th.random_start:
                    ops.append(eng.pgd_random_start(pv, eps, th.ball, (s + i) & 0xFFFFFFFF, th.box, valid=b.valids[i]))
                else:
                    ops.append(eng.make_operand(pv))
                    if not b.attacked[i]:                                   # a view that is not attacked: delta 0, never stepped
                        pv.delta.zero_()
            for k in range(steps):
                self._forward(b, ops, L.MODE_DATA, True)
                if self.task == "vqa":
                    b.loss.backward(b.view, ops[0], L.MODE_DATA, dpatches=b.view.gpatch)
                else:
                    b.loss.backward(b.view, None, L.MODE_DATA, dpatches=b.attacked)
                for i, pv in enumerate(b.views):
                    if b.attacked[i]:
                        ops[i] = eng.pgd_step_ball(pv, lr, eps, th.direction, th.ball, th.box, first=k == 0 and not th.random_start,
                                                   out=pv.patchesT, valid=b.valids[i])
            self._forward(b, ops, L.MODE_INFER, False)                      # the per-sample loss of delta_K
            col = self._loss_column(b)
            for i, pv in enumerate(b.views):                                # (every view of a sample takes the same decision)
                eng.pgd_keep_worst(col, b.best_score[i], b.best_restart[i], r, pv.delta, b.best_delta[i], ops[i], b.best_op[i],
                                   rows_per_decision=b.rows_per_decision)
        return self._results(b, b.best_op)

    def _delta_images(self, b):
        eng = self.eng
        if self.task == "vqa":
            return eng.patches_to_image(b.best_delta[0], b.view)
        d0, d1 = pair_images(eng, b.view, b.best_delta, b.shapes)
        return d0.contiguous(), d1.contiguous()

    @staticmethod
    def _threat(norm, step_rule, random_start, box, seed):
        return ThreatModel(norm, "normalised" if norm == "l2" else step_rule, random_start, box, seed)

    @staticmethod
    def _check(steps, restarts):
        if int(steps) < 0 or int(restarts) < 1:
            raise ValueError(f"steps must be >= 0 and restarts >= 1 (got {steps}, {restarts})")

    def attack(self, batch, eps, norm="linf", steps=10, step_size=None, step_rule="sign", random_start=True, restarts=1, box=(-1.0, 1.0), seed=0):
        """PGD on the image of a VQA batch (``text_ids``, ``text_masks``, ``image``, ``vqa_labels``, ``vqa_scores``) or on the images of an
        NLVR2 batch (``image_0``, ``image_1``, ``answers``; the model's ``attack_idx`` selects which image is attacked).  Float images or
        batches of the byte feed.  Per restart: K = `steps` x (forward, data-gradient backward, ``pgd_step_ball``) from a random start
        (or from 0), then one inference forward for the per-sample loss of delta_K; the restart with the largest loss is kept per sample.
        step_size None: 2.5 eps / steps.  box: the valid pixel range (None: no box); (-1, 1) is the pixelbert normalisation's.

        Returns a dict of device tensors: ``delta`` [B,3,H,W] (NLVR2: a pair), ``clean_loss`` / ``adv_loss`` [B], ``clean_pred`` /
        ``adv_pred`` [B] int32, ``clean_score`` / ``adv_score`` [B] (VQA: the soft target at the predicted answer; NLVR2: 1 where the
        prediction is right), ``best_restart`` [B] int32."""
        self._check(steps, restarts)
        th = self._threat(norm, step_rule, random_start, box, seed)
        with self._eval():
            b = self._bind(batch)
            adv = self._attack_bound(b, eps, th, int(steps), step_size, int(restarts), seed)
            return self._pack(b, adv, self._delta_images(b))

    @staticmethod
    def _pack(b, adv, delta):
        return {"delta": delta, "clean_loss": b.clean[0], "clean_pred": b.clean[1], "clean_score": b.clean[2],
                "adv_loss": adv[0], "adv_pred": adv[1], "adv_score": adv[2], "best_restart": b.best_restart[0].clone()}

    def curve(self, batches, eps, norm="linf", steps=10, step_size=None, step_rule="sign", random_start=True, restarts=1, box=(-1.0, 1.0), seed=0):
        """Score versus eps over an iterable of batches (a list, a DataLoader).  Returns one dict per eps, in the order given: ``eps``, ``n``,
        ``clean_score`` / ``robust_score`` (VQA score, or NLVR2 accuracy), ``flip_rate`` (share of samples whose prediction changed),
        ``clean_loss`` / ``adv_loss`` (means).  The clean forward runs once per batch; the sums stay on the device and are read once."""
        self._check(steps, restarts)
        eps = [float(e) for e in eps]
        th = self._threat(norm, step_rule, random_start, box, seed)
        acc = torch.zeros(len(eps), 5, dtype=torch.float64, device=self.eng.device)
        n = 0
        with self._eval():
            for batch in batches:
                b = self._bind(batch)
                n += b.B
                for j, e in enumerate(eps):
                    adv = self._attack_bound(b, e, th, int(steps), step_size, int(restarts), seed)
                    acc[j] += torch.stack([b.clean[2].sum(), adv[2].sum(), (adv[1] != b.clean[1]).sum().to(torch.float32), b.clean[0].sum(),
                                           adv[0].sum()]).to(torch.float64)
        host = (acc / max(n, 1)).cpu().tolist()
        keys = ("clean_score", "robust_score", "flip_rate", "clean_loss", "adv_loss")
        return [dict({"eps": e, "n": n}, **dict(zip(keys, row))) for e, row in zip(eps, host)]
