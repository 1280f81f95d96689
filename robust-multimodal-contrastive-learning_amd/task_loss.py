"""One loss object per objective - MoCo / InfoNCE, Barlow-Twins, VQA, NLVR2 - for the training loss, the PGD image attack and the greedy
text attack: it owns the head buffers and the chain "pooled cls rows -> task head -> loss -> gradient at the cls rows".  A *view* is what
one encoder pass runs on: ``PassBuffers``, for NLVR2 the ``Nlvr2Pass`` of the image pair.  DESIGN.md "Objective loss objects"."""
from __future__ import annotations

import torch

from . import _lib as L

HEAD_ROWS = 256                       # include/rmcl.h: the classifier launchers take at most 256 rows


class Nlvr2Pass:
    """The encoder passes of one NLVR2 batch.  Pair form (config["nlvr2_pair_pass"], default on): ONE pass of 2B sequences, sample 2b =
    (text b, image_0[b], token type 1), 2b + 1 = (text b, image_1[b], token type 2) - its pooled cls [2B, D] IS the [B, 2D] input of
    nlvr2_classifier and the head's [B, 2D] gradient IS the pass's cls gradient.  Two-pass form: the reference's two infer calls
    (image_token_type_idx 1 and 2), one pass of B sequences each, the cls halves concatenated / split by copies."""

    patchesT = None                   # (where a loss object asks a view for its candidates' operand: the pass has its own ``ops``)

    def __init__(self, eng, views, B, pair):
        self.eng, self.views, self.B, self.pair = eng, views, B, pair
        self.ops = [None] * len(views)

    @classmethod
    def bind(cls, pl_module, batch, tag):
        eng = pl_module.engine
        img0, img1 = batch["image_0"][0], batch["image_1"][0]
        B = int(img0.shape[0])
        if pl_module.hparams.config.get("nlvr2_pair_pass", True):
            if not torch.is_tensor(img0) or not torch.is_tensor(img1):
                # byte feeds: the pair pass interleaves the two images pixel by pixel (Engine.bind_pair), which needs float pixels
                from .attack.pgd_attack_vilt import device_image
                img0, img1 = device_image(eng, img0), device_image(eng, img1)
            return cls(eng, [eng.bind_pair(batch["text_ids"], batch["text_masks"], img0, img1, tag=tag)], B, True)
        views = []
        for t, img in ((1, img0), (2, img1)):                  # geometry drawn in the reference's order: image_0, then image_1
            pv = eng.bind_batch(batch["text_ids"], batch["text_masks"], img, tag=f"{tag}_{t}")
            pv.d.img_type = t
            views.append(pv)
        return cls(eng, views, B, False)

    def twin(self, tag):
        """the same pairs in buffers of their own (the attacked pass): shares the text, the clean patch rows and the geometry"""
        vs = []
        for i, pv in enumerate(self.views):
            pt = self.eng.twin(pv, f"{tag}_{i}")
            pt.text_ids, pt.text_mask, pt.patches32 = pv.text_ids, pv.text_mask, pv.patches32
            vs.append(pt)
        return Nlvr2Pass(self.eng, vs, self.B, self.pair)

    def text_of(self, ids, masks):
        """B sentences (ids, masks on the device) as the text of one view: the pair form reads sentence b in sequences 2b and 2b + 1"""
        if self.pair:
            ids, masks = ids.repeat_interleave(2, dim=0), masks.repeat_interleave(2, dim=0)
        return ids.contiguous(), masks.contiguous()

    def set_text(self, ids, masks):
        for pv in self.views:
            pv.text_ids, pv.text_mask = self.text_of(ids, masks)

    def clean_operands(self, full_buffer=True):
        self.ops = [self.eng.make_operand(pv, out=pv.patchesT_full if full_buffer else None) for pv in self.views]
        return self.ops

    def forward(self, mode, wgrad):
        eng = self.eng
        for pv, op in zip(self.views, self.ops):
            eng.encoder_forward(pv, key=False, mode=mode, patchesT=op, cls_tail=True)
            eng.heads_forward(pv, key=False, want_q=False, wgrad=wgrad)
        if self.pair:
            return self.views[0].cls.view(self.B, -1)                         # [2B, D] -> [B, 2D]: no copy
        return torch.cat([pv.cls for pv in self.views], dim=1)

    def backward(self, dcls2, mode, with_grads, dpatches=False, dtext=None, skip=()):
        """dpatches: per view (or for all) whether the patch gradient is wanted; dtext: the text gradient's target; skip: views not run"""
        eng = self.eng
        D = self.views[0].d.D
        for i, (pv, op) in enumerate(zip(self.views, self.ops)):
            if i in skip:
                continue
            dc = dcls2.view(2 * self.B, D) if self.pair else dcls2[:, i * D:(i + 1) * D].contiguous()
            eng.heads_backward(pv, None, dc, with_grads=with_grads)
            want = dpatches if isinstance(dpatches, bool) else dpatches[i]
            eng.encoder_backward(pv, mode, op, pv.dcls, cls_only=True, dpatches=pv.gpatch if want else None, dtext=dtext)


class TaskLoss:
    """``forward`` returns the per-row loss terms and leaves ``feats`` (what the reference's get_grad returns third).  ``K``: the loss is
    divided by K; ``scale``: a gradient scale other than the objective's own; ``wgrad``: Engine.heads_forward; ``before_loss`` runs
    between the pooler and the loss.  ``defer``: the backward comes later, as ``backward(..., g=grad_out)``: ``value`` and the statistics
    go to tensors of their own, and a loss kernel that takes the incoming gradient as a device scalar (VQA, NLVR2) runs again then.
    A backward forms weight gradients in MODE_FULL, none in MODE_DATA."""
    want_q = False            # the pooler pass also writes the MoCo projection
    stash_pooler = False      # the pooler input is kept also where no weight gradient follows (the contrastive objectives outside PGD)

    def __init__(self, pl_module):
        self.pl, self.eng = pl_module, pl_module.engine

    def scale(self, view, K=1):
        return 1.0 / K

    def _fresh(self, n):
        return torch.empty(n, dtype=torch.float32, device=self.eng.device)

    def forward(self, view, op, mode, K=1, want_grad=True, scale=None, wgrad=None, before_loss=None, **kw):
        cls = self.encode(view, op, mode, (mode == L.MODE_FULL or self.stash_pooler) if wgrad is None else wgrad)
        if before_loss is not None:
            before_loss()
        return self.loss_forward(view, cls, self.scale(view, K) if scale is None else scale, want_grad, **kw)

    def encode(self, view, op, mode, wgrad):
        self.eng.encoder_forward(view, key=False, mode=mode, patchesT=op, cls_tail=True)
        self.pool(view, wgrad)
        return view.cls

    def pool(self, view, wgrad):
        self.eng.heads_forward(view, key=False, want_q=self.want_q, wgrad=wgrad)

    def head_backward(self, view, with_grads, g=None):
        """loss -> head -> pooler: leaves the gradient at the encoder's cls rows in ``view.dcls``"""
        dq, dcls = self.loss_backward(view, with_grads, g)
        self.eng.heads_backward(view, dq, dcls, with_grads=with_grads)

    def backward(self, view, op, mode, g=None, dpatches=None, dtext=None):
        self.head_backward(view, mode == L.MODE_FULL, g)
        self.eng.encoder_backward(view, mode, op, view.dcls, cls_only=True, dpatches=dpatches, dtext=dtext)

    def candidate_rows(self, cview, ctx, owner, n_real):
        """The text attack's scoring: candidate r through the encoder and the head against the targets of sample owner[r] (gathered on
        the device); one transfer brings back (row terms of the batch `ctx`, row terms of the n_real candidates) as host lists."""
        cls = self.encode(cview, cview.patchesT, L.MODE_INFER, self.stash_pooler)
        Bn = int(ctx.shape[0])
        own = torch.tensor(owner[:n_real], device=self.eng.device)
        rows = self._fresh(Bn + n_real)
        rows[:Bn].copy_(ctx)
        self.candidate_terms(cls[:n_real], own, rows[Bn:])
        host = rows.cpu().tolist()
        return host[:Bn], host[Bn:]


class InfoNceLoss(TaskLoss):
    """MoCo: pooler + projection head, InfoNCE of q against (k, queue) - CE(label 0), mean over the batch (:152-158); gradient wrt q
    only.  ``k``: keys to copy into the view first; ``clean_out``: dict for the clean-query statistics; ``metrics``: Engine.infonce."""
    want_q = True
    stash_pooler = True

    def __init__(self, pl_module, metrics=True):
        super().__init__(pl_module)
        self.metrics = metrics

    def scale(self, view, K=1):
        return 1.0 / (view.B * K)

    def loss_forward(self, pv, cls, grad_scale, want_grad, defer=False, k=None, clean_out=None):
        if k is not None and pv.k.data_ptr() != k.data_ptr():
            pv.k.copy_(k)
        self.eng.infonce(pv, grad_scale, want_dq=want_grad, metrics=self.metrics)
        if clean_out is not None:
            clean_out["prediction"], clean_out["q"] = pv.rows[:, 1].clone(), pv.q.clone()
        self.feats = pv.q
        if defer:
            self.value, self.held = pv.loss_sum.clone().reshape(()), (pv.dq.clone() if want_grad else None)
        return pv.rows[:, 0]

    def loss_backward(self, pv, with_grads, g=None):
        return (pv.dq if g is None else self.held * g.to(self.held.dtype)), None

    def candidate_rows(self, pc, ctx, owner, n_real):
        """split_forward (:454-492): candidates through the encoder, per-row CE against the same keys."""
        cec = self.forward(pc, pc.patchesT, L.MODE_INFER, want_grad=False, scale=0.0)[:n_real].cpu().tolist()
        return ctx.cpu().tolist(), cec


class BarlowLoss(TaskLoss):
    """Barlow-Twins: z = barlowtwins_head(cls_feats) in the buffers `tag`, loss = on_diag + adv_lr * off_diag of c = z^T zk / denom
    (the reference uses its `adv_lr` hyper-parameter as the redundancy weight).  The BatchNorms run in the module's mode - an attack's
    deep copy of the head keeps the train / eval flag (pgd_attack_vilt.py:189) - and only the module's own head (``track``) updates the
    running estimates.  ``denom``: None = the local batch (the attacks).  Row terms: the projection rows (``candidate_rows``)."""
    stash_pooler = True
    feats = None              # (the projections: the consumer's own copy of the row terms)

    def __init__(self, pl_module, tag, zk=None, track=False, denom=None, reduce_c=None):
        super().__init__(pl_module)
        self.tag, self.zk, self.track, self.denom, self.reduce_c = tag, zk, track, denom, reduce_c
        self.training = bool(pl_module.training)

    def project(self, pv, cls):
        """the projection of pooled cls rows alone (also the key side: k = head(infer(clean)), objectives.py:460-462)"""
        self.bb = self.eng.bt_bufs(pv.B, self.tag)
        return self.eng.bt_forward(self.bb, cls, self.training, track=self.track)

    def loss_forward(self, pv, cls, grad_scale, want_grad, defer=False):
        self.project(pv, cls)
        self.loss2 = self.eng.bt_loss(self.bb, self.zk, float(pv.B if self.denom is None else self.denom), self.pl.adv_lr, grad_scale,
                                      want_dz=want_grad, reduce_c=self.reduce_c)
        if defer:
            self.on_diag, self.red = self.loss2[0].clone(), self.pl.adv_lr * self.loss2[1]
            self.value, self.held = (self.on_diag + self.red).reshape(()), (self.bb.dz.clone() if want_grad else None)
        return self.bb.z

    def loss_backward(self, pv, with_grads, g=None):
        bb = self.eng.bt_bufs(pv.B, self.tag)
        dz = bb.dz if g is None else self.held * g.to(self.held.dtype)
        return None, self.eng.bt_backward(bb, dz, training=self.training, with_grads=with_grads)

    def candidate_rows(self, pc, ctx, owner, n_real):
        """split_forward (:670-707).  Candidates go through encoder + head as ONE batch of n_real rows (BatchNorm statistics
        over exactly those rows); then, sample by sample and candidate by candidate, row i of the projection matrix is
        replaced and the loss of the whole matrix re-evaluated.  `t_save = ori_z[i]` (:691) is a view, so row i keeps its LAST
        candidate while later samples are scored (same reference behaviour as the MoCo attack); the comparison baseline is
        the loss of the UNMODIFIED matrix for every sample (:684-688).  All n_real + 1 losses are produced on the device
        and read back once: ([loss of the unmodified matrix], candidate losses)."""
        eng = self.eng
        cls = self.encode(pc, pc.patchesT, L.MODE_INFER, True)
        zc = eng.bt_forward(eng.bt_bufs(n_real, self.tag + "_cand"), cls[:n_real].contiguous(), training=self.training, track=False)
        Z = ctx.clone()
        Bn = int(Z.shape[0])
        vals = torch.empty(n_real + 1, 2, device=Z.device)
        lam = self.pl.adv_lr
        eng.bt_loss_of(Z, self.zk, Bn, float(Bn), lam, 1.0, vals[0])
        for r in range(n_real):
            Z[owner[r]].copy_(zc[r])
            eng.bt_loss_of(Z, self.zk, Bn, float(Bn), lam, 1.0, vals[1 + r])
        v = vals.cpu().double()
        loss = (v[:, 0] + lam * v[:, 1]).tolist()
        return loss[:1], loss[1:]


class VqaLoss(TaskLoss):
    """VQA: vqa_classifier on the pooled cls rows, BCE-with-logits x vqav2_label_size (objectives.py:861-896), in the VqaBuffers `vb`.
    The label / score tables are in `vb` by the time of the loss (Engine.vqa_targets).  Row terms: the per-row BCE sums."""

    def __init__(self, pl_module, vb):
        super().__init__(pl_module)
        self.vb = vb

    def scale(self, view, K=1):
        return 1.0                                              # NOT divided by K (pgd_attack_vilt.py:444-460)

    def loss_forward(self, pv, cls, grad_scale, want_grad, defer=False):
        self.logits, self.feats = self.eng.vqa_forward(self.vb, cls), cls
        self.stats = self.eng.vqa_bce(self.vb, grad_scale, want_dz=want_grad and not defer, loss2=self._fresh(2) if defer else None)
        self.value = self.stats[0].reshape(())
        return self.vb.rows[:, 0]

    def loss_backward(self, pv, with_grads, g=None):
        if g is not None:                                       # the deferred backward: d loss / d logits x the incoming gradient, on the device
            self.eng.vqa_bce(self.vb, 1.0, want_dz=True, scale_dev=g.to(torch.float32).reshape(1).contiguous(), loss2=self._fresh(2))
        return None, self.eng.vqa_backward(self.vb, self.vb.dz, with_grads=with_grads)

    def candidate_terms(self, cls, own, out):
        self.rows_of(self.eng, cls, self.vb.labels.index_select(0, own), self.vb.scores.index_select(0, own), self.vb.A, out)

    @staticmethod
    def rows_of(eng, cls, labels, scores, A, out=None, tag="txtatk_cand"):
        """Per-row BCE sums (rmcl_vqa_bce rows[:, 0]) of vqa_classifier(cls [R, D]) against the label / score tables [R, A] (device, one
        row per cls row), R of any size: the head launcher takes at most 256 rows, so the rows go through it in chunks.  Every row of
        the head and of the loss is independent of the others, so the chunking changes no value.  Returns `out` [R] on the device."""
        R = int(cls.shape[0])
        out = torch.empty(R, dtype=torch.float32, device=eng.device) if out is None else out
        for s, e in ((s, min(R, s + HEAD_ROWS)) for s in range(0, R, HEAD_ROWS)):
            vb = eng.vqa_bufs(e - s, tag)
            vb.labels, vb.scores, vb.A = labels[s:e].contiguous(), scores[s:e].contiguous(), A
            eng.vqa_forward(vb, cls[s:e])
            eng.vqa_bce(vb, 1.0, want_dz=False)
            out[s:e].copy_(vb.rows[:, 0])
        return out


vqa_candidate_rows = VqaLoss.rows_of


class Nlvr2Loss(TaskLoss):
    """NLVR2: CE(nlvr2_classifier(cat(cls(image_0, type 1), cls(image_1, type 2))), answers) (objectives.py:1002-1060) in the Nlvr2Buffers
    `nb` (labels bound by the time of the loss).  Its view is an ``Nlvr2Pass``, which runs the pooler with each encoder pass on its own
    ``ops``.  ``ref``: Engine.nlvr2_ce; ``skip``: Nlvr2Pass.backward.  Row terms: the per-pair CE."""

    def __init__(self, pl_module, nb, ref=None, skip=()):
        super().__init__(pl_module)
        self.nb, self.ref, self.skip = nb, ref, skip

    def encode(self, npass, op, mode, wgrad):
        return npass.forward(mode, wgrad)

    def loss_forward(self, npass, cls2, grad_scale, want_grad, defer=False):
        self.logits, self.feats = self.eng.nlvr2_forward(self.nb, cls2), cls2
        self.stats = self.eng.nlvr2_ce(self.nb, grad_scale, want_dz=want_grad and not defer, ref=self.ref, stats=self._fresh(3) if defer else None)
        self.value = self.stats[0].reshape(())
        return self.nb.rows

    def backward(self, npass, op, mode, g=None, dpatches=False, dtext=None):
        if g is not None:
            self.eng.nlvr2_ce(self.nb, 1.0, want_dz=True, scale_dev=g.to(torch.float32).reshape(1).contiguous(), stats=self._fresh(3))
        dcls2 = self.eng.nlvr2_backward(self.nb, self.nb.dz, with_grads=mode == L.MODE_FULL)
        npass.backward(dcls2, mode, mode == L.MODE_FULL, dpatches, dtext, self.skip)

    def candidate_terms(self, cls2, own, out, tag="txtatk_cand"):
        """Per-row CE (rmcl_nlvr2_ce rows) of nlvr2_classifier(cls2 [R, 2 hidden]) against the owners' labels, in chunks of 256."""
        eng, cls2, labels = self.eng, cls2.contiguous(), self.nb.labels.index_select(0, own)
        for s, e in ((s, min(len(cls2), s + HEAD_ROWS)) for s in range(0, len(cls2), HEAD_ROWS)):
            nb = eng.nlvr2_bufs(e - s, tag)
            nb.labels.copy_(labels[s:e])
            eng.nlvr2_forward(nb, cls2[s:e])
            eng.nlvr2_ce(nb, 1.0, want_dz=False)
            out[s:e].copy_(nb.rows)
