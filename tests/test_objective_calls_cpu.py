"""CPU: the sequence of engine calls behind every objective, PGD image attack and greedy text attack, against a recorded list.

A recording stand-in for ``Engine`` (small CPU tensors, deterministic fill values for whatever the host reads back) and a minimal
``pl_module`` drive the public entry points - ``compute_vqa`` / ``compute_vqa_attack`` / ``compute_nlvr2`` / ``compute_nlvr2_attack`` /
``compute_barlowtwins_contrastive`` with ``.backward()`` on the returned losses, every ``attack_patches`` / ``attack_pairs`` /
``pgd_attack``, ``get_grad`` / ``score`` / ``adv_attack_samples`` of the four text attacks - and every engine call is written down with
its arguments: scalars as they are, buffer objects by class, tag and batch size, tensors by the buffer attribute they are (else by
shape and dtype), plus ``after_backward`` and the keys logged.  tests/golden/objective_calls.json holds, per scenario, the length and
the SHA-256 of that list, and the list itself for the scenarios named in FULL.  The Python that issues the calls may be reorganised
freely; what reaches the device - which call, on which buffers, with which flags, in which order - may not change unnoticed.

Not written down: the pure buffer look-ups (``bufs`` / ``bt_bufs`` / ``vqa_bufs`` / ``nlvr2_bufs`` return cached objects and launch
nothing; every use of such a buffer names its tag anyway).  ``compute_moco_contrastive`` needs HIP stream objects and is covered by the
GPU goldens and the pass_log test.

``python -m tests.test_objective_calls_cpu --record`` rewrites the fixture."""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd import runtime as RT
from rmcl_amd.attack import greedy_attack_vilt as GA
from rmcl_amd.attack import pgd_attack_vilt as PA
from rmcl_amd.attack import word_substitution as WS
from rmcl_amd.vilt.modules import objectives as OBJ
from tests.golden_util import GOLDEN

FIXTURE = os.path.join(GOLDEN, "objective_calls.json")
SENTENCES = ["a big dog and a small cat run on the green field near the house",
             "the man and the woman walk on the street with a child holding a red ball",
             "two dogs jump over a table in the house",
             "a lady is sitting in a boat looking at the kid playing with some puppy near a car"]
B, LT, D, PROJ, H3, S, PS, NLAB = 4, 24, 4, 3, 5, 4, 2, 7
NP, PK = (S // PS) ** 2, 3 * PS * PS
# scenarios whose whole list is kept in the fixture (the rest: length and SHA-256)
FULL = ("vqa/train", "vqa_attack/img/K2/train", "nlvr2_attack/two_pass/both/idx10/K2/train", "bt/both/K1/train", "pgd/moco/K2/hooks",
        "greedy/nlvr2/pair/get_grad_score")


# ---- the recording engine --------------------------------------------------------------------------------------------------------------
class _Buf:
    def __init__(self, kind, tag, Bn):
        self.name, self.B = f"{kind}:{tag}:{Bn}", Bn


def _f32(*s):
    return torch.zeros(*s, dtype=torch.float32)


class FakeEngine:
    def __init__(self, trace, dtype=L.BF16, pgd_dtype=None):
        self.trace, self.objs, self.cache, self.n = trace, [], {}, 0
        self.device, self.dtype, self.pgd_dtype, self.exact, self.irtr = torch.device("cpu"), dtype, pgd_dtype, False, False
        self.cfg = {"hidden_size": D, "image_size": S, "patch_size": PS}

    # -- naming ---------------------------------------------------------------------------------------------------------------------
    def name_ptr(self, ptr, shape=None):
        for o in self.objs:
            for a, v in vars(o).items():
                if torch.is_tensor(v) and v.numel() and v.data_ptr() == ptr:
                    same = shape is None or tuple(v.shape) == tuple(shape)
                    return f"{o.name}.{a}" + ("" if same else str(list(shape)))
        return None

    def name(self, x):
        if x is None or isinstance(x, (bool, int, str)):
            return repr(x)
        if isinstance(x, float):
            return repr(round(x, 9))
        if isinstance(x, _Buf):
            return x.name
        if torch.is_tensor(x):
            n = self.name_ptr(x.data_ptr(), x.shape) if x.numel() else None
            return n or f"{str(x.dtype).replace('torch.', '')}{list(x.shape)}"
        if isinstance(x, (list, tuple)):
            return "[" + ",".join(self.name(v) for v in x) + "]"
        if callable(x):
            return "fn"
        return type(x).__name__

    def rec(self, what, *args, **kw):
        self.trace.append(what + "(" + ",".join([self.name(a) for a in args] + [f"{k}={self.name(v)}" for k, v in kw.items()]) + ")")

    def fill(self, t):
        """deterministic values in (0.05, 1.05) for what the host reads back and decides on"""
        self.n += 1
        v = ((torch.arange(t.numel(), dtype=torch.int64) * 7919 + self.n * 104729) % 1009).to(torch.float32) / 1009.0 + 0.05
        t.copy_(v.view(t.shape))

    def obj(self, kind, tag, Bn, make):
        key = (kind, tag, Bn)
        if key not in self.cache:
            o = self.cache[key] = _Buf(kind, tag, Bn)
            make(o)
            self.objs.append(o)
        return self.cache[key]

    # -- pass buffers ---------------------------------------------------------------------------------------------------------------
    def bufs(self, Bn, tag="moco", dtype=None, P=None):
        def make(o):
            o.dtype = self.dtype if dtype is None else dtype
            o.d = SimpleNamespace(B=Bn, L=LT, P=NP, D=D, patch_k=PK, proj=PROJ, img_type=0)
            o.geom = None
            tdt = torch.float32 if o.dtype == L.F32 else torch.bfloat16
            o.xn = _f32(Bn * (LT + 1 + NP), D)
            o.patches32, o.delta, o.delta_prev = _f32(Bn * NP, PK), _f32(Bn * NP, PK), _f32(Bn * NP, PK)
            o.patchesT, o.patchesT_full, o.gpatch = (torch.zeros(Bn * NP, PK, dtype=tdt) for _ in range(3))
            o.cls, o.dcls, o.q, o.k, o.dq, o.rows = _f32(Bn, D), _f32(Bn, D), _f32(Bn, PROJ), _f32(Bn, PROJ), _f32(Bn, PROJ), _f32(Bn, 10)
            o.loss_ring, o.loss_i = _f32(32), 0
            o.loss_sum = o.loss_ring[0:1]
            o.text_ids = o.text_mask = None
        return self.obj("Pass", tag, Bn, make)

    def _text(self, pb, ids, masks):
        pb.text_ids, pb.text_mask = ids.to(torch.int64).contiguous(), masks.to(torch.int64).contiguous()

    def bind_batch(self, text_ids, text_mask, image, tag="moco", select=None):
        self.rec("bind_batch", text_ids, text_mask, image, tag=tag)
        pb = self.bufs(int(image.shape[0]), tag)
        pb.d.img_type = 0
        self._text(pb, text_ids, text_mask)
        return pb

    def bind_pair(self, text_ids, text_mask, image0, image1, tag="nlvr2"):
        self.rec("bind_pair", text_ids, text_mask, image0, image1, tag=tag)
        pb = self.bufs(2 * int(image0.shape[0]), tag)
        pb.d.img_type = -1
        self._text(pb, text_ids.repeat_interleave(2, dim=0), text_mask.repeat_interleave(2, dim=0))
        return pb

    def twin(self, pb, tag, dtype=None, owner=None):
        self.rec("twin", pb, tag, dtype=dtype, owner=owner)
        pv = self.bufs(pb.B if owner is None else int(owner.numel()), tag, dtype)
        pv.d.img_type = pb.d.img_type
        return pv

    def bind_text(self, like, text_ids, text_mask, tag):
        self.rec("bind_text", like, text_ids, text_mask, tag)
        pv = self.bufs(like.B, tag)
        pv.d.img_type = like.d.img_type
        self._text(pv, text_ids, text_mask)
        pv.patches32 = like.patches32
        return pv

    def pgd_bufs(self, pb):
        self.rec("pgd_bufs", pb)
        if self.pgd_dtype is None or self.pgd_dtype == pb.dtype:
            return pb
        pp = self.bufs(pb.B, "pgd_f32", self.pgd_dtype)
        pp.text_ids, pp.text_mask, pp.patches32 = pb.text_ids, pb.text_mask, pb.patches32
        pp.delta, pp.delta_prev, pp.k = pb.delta, pb.delta_prev, pb.k
        return pp

    def lanes(self, pb, n=None):
        self.rec("lanes", pb)
        return None

    def make_operand(self, pb, d1=None, d2=None, out=None):
        self.rec("make_operand", pb, d1, d2, out=out)
        return pb.patchesT if out is None else out

    def patches_to_image(self, pat, pb):
        self.rec("patches_to_image", pat, pb)
        return _f32(pb.B, 3, S, S)

    def zero_scalar(self, pb, log=True):
        if log:
            self.rec("zero_scalar", pb)
        if pb.loss_i == pb.loss_ring.numel():
            pb.loss_i = 0
        pb.loss_sum = pb.loss_ring[pb.loss_i:pb.loss_i + 1]
        pb.loss_i += 1
        return pb.loss_sum

    def delta_channel_norm(self, pb, out=None):
        """(the one call the objectives once made past the engine: written down the same way in both forms)"""
        if out is None:
            out = self.zero_scalar(pb)
        self.trace.append(f"delta_channel_norm({self.name_ptr(pb.delta.data_ptr())},{self.name_ptr(out.data_ptr()) or 'f32[1]'})")
        return out

    # -- encoder and pooler ---------------------------------------------------------------------------------------------------------
    def encoder_forward(self, pb, key, mode, patchesT, cls_tail=False):
        self.rec("encoder_forward", pb, key=key, mode=mode, patchesT=patchesT, cls_tail=cls_tail, ids=list(pb.text_ids.shape))

    def heads_forward(self, pb, key, want_q=True, wgrad=True):
        self.rec("heads_forward", pb, key=key, want_q=want_q, wgrad=wgrad)

    def infonce(self, pb, grad_scale, want_dq, metrics=True):
        self.zero_scalar(pb, log=False)
        self.rec("infonce", pb, grad_scale, want_dq=want_dq, metrics=metrics)
        self.fill(pb.rows)

    def heads_backward(self, pb, dq, dcls_extra, with_grads):
        self.rec("heads_backward", pb, dq, dcls_extra, with_grads=with_grads)

    def encoder_backward(self, pb, mode, patchesT, dxn, cls_only, dpatches, dtext=None):
        self.rec("encoder_backward", pb, mode, patchesT, dxn, cls_only=cls_only, dpatches=dpatches, dtext=dtext)
        if dtext is not None:
            self.fill(dtext)

    def pgd_step(self, pb, lr, eps, first=False, out=None, sum_prev=False):
        self.rec("pgd_step", pb, lr, eps, first=first, out=out, sum_prev=sum_prev)

    def word_saliency(self, g, spans, L_, row0=0, row_step=1, out=None):
        self.rec("word_saliency", g, list(spans.shape), L_, row0, row_step)
        out = _f32(int(spans.shape[0]), int(spans.shape[1]))
        self.fill(out)
        return out

    # -- Barlow-Twins ---------------------------------------------------------------------------------------------------------------
    def bt_bufs(self, Bn, tag):
        def make(o):
            o.z, o.dz, o.dcls, o.rows, o.loss2 = _f32(Bn, H3), _f32(Bn, H3), _f32(Bn, D), _f32(Bn, 3), _f32(2)
        return self.obj("Bt", tag, Bn, make)

    def bt_forward(self, bb, cls, training, track):
        self.rec("bt_forward", bb, cls, training=training, track=track)
        self.fill(bb.z)
        return bb.z

    def bt_backward(self, bb, dz, training, with_grads):
        self.rec("bt_backward", bb, dz, training=training, with_grads=with_grads)
        return bb.dcls

    def bt_loss(self, bb, zk, denom, lam, grad_scale, want_dz, reduce_c=None):
        self.rec("bt_loss", bb, zk, denom, lam, grad_scale, want_dz=want_dz, reduce_c=reduce_c)
        self.fill(bb.loss2)
        return bb.loss2

    def bt_loss_of(self, z, zk, Bn, denom, lam, grad_scale, loss2, reduce_c=None):
        self.rec("bt_loss_of", z, zk, Bn, denom, lam, grad_scale, list(loss2.shape), reduce_c=reduce_c)
        self.fill(loss2)

    def bt_pair_metrics(self, bb, zk):
        self.rec("bt_pair_metrics", bb, zk)
        return bb.rows

    # -- VQA / NLVR2 heads ----------------------------------------------------------------------------------------------------------
    def _classifier(self, kind, Bn, tag, N, Din, rows_shape):
        def make(o):
            o.logits_p = _f32(Bn, 64)
            o.logits, o.dz, o.dcls, o.rows = o.logits_p[:, :N], _f32(Bn, 64), _f32(Bn, Din), _f32(*rows_shape)
            o.argmax = torch.zeros(Bn, dtype=torch.int32)
            o.loss2, o.stats, o.labels, o.scores, o.A = _f32(2), _f32(3), torch.zeros(Bn, dtype=torch.int32), None, 0
        return self.obj(kind, tag, Bn, make)

    def vqa_bufs(self, Bn, tag):
        vb = self._classifier("Vqa", Bn, tag, NLAB, D, (Bn, 2))
        if vb.A == 0:
            vb.labels = None
        return vb

    def vqa_targets(self, vb, labels, scores):
        self.rec("vqa_targets", vb, [len(r) for r in labels], [len(r) for r in scores])
        vb.A = max([1] + [len(r) for r in labels])
        vb.labels, vb.scores = torch.full((vb.B, vb.A), -1, dtype=torch.int32), _f32(vb.B, vb.A)
        return vb

    def vqa_forward(self, vb, cls):
        self.rec("vqa_forward", vb, cls, tables=[self.name(vb.labels), self.name(vb.scores), vb.A])
        return vb.logits

    def vqa_bce(self, vb, grad_scale, want_dz, scale_dev=None, loss2=None):
        self.rec("vqa_bce", vb, grad_scale, want_dz=want_dz, scale_dev=scale_dev, loss2=loss2)
        self.fill(vb.rows)
        loss2 = vb.loss2 if loss2 is None else loss2
        self.fill(loss2)
        return loss2

    def vqa_backward(self, vb, dz, with_grads):
        self.rec("vqa_backward", vb, dz, with_grads=with_grads)
        return vb.dcls

    def vqa_targets_dense(self, vb):
        self.rec("vqa_targets_dense", vb)
        return _f32(vb.B, NLAB)

    def nlvr2_bufs(self, Bn, tag):
        return self._classifier("Nlvr2", Bn, tag, 2, 2 * D, (Bn,))

    def nlvr2_labels(self, nb, answers):
        self.rec("nlvr2_labels", nb, len(answers))
        nb.labels.copy_(torch.tensor([int(a) for a in answers], dtype=torch.int32))
        return nb.labels

    def nlvr2_forward(self, nb, cls2):
        self.rec("nlvr2_forward", nb, cls2)
        return nb.logits

    def nlvr2_ce(self, nb, grad_scale, want_dz, scale_dev=None, ref=None, stats=None):
        self.rec("nlvr2_ce", nb, grad_scale, want_dz=want_dz, scale_dev=scale_dev, ref=ref, stats=stats)
        self.fill(nb.rows)
        stats = nb.stats if stats is None else stats
        self.fill(stats)
        return stats

    def nlvr2_backward(self, nb, dz, with_grads):
        self.rec("nlvr2_backward", nb, dz, with_grads=with_grads)
        return nb.dcls


class FakeModule:
    def __init__(self, task, trace, K=2, training=True, image_view=True, text_view=False, pgd_f32=False, pair=True, attack_idx=(1, 1)):
        res = {k: os.path.join(GOLDEN, f"toy_{v}.txt") for k, v in (("tokenizer", "vocab"), ("embedding_path", "counter_fitted"),
                                                                    ("stopwords", "stopwords"))}
        cfg = dict(adv_steps_img=K, adv_lr_img=0.5, adv_max_norm_img=0.25, max_image_len=-1, max_text_len=LT, n_candidates=3, max_loops=2,
                   vocab_size=30522, seed=3, attack_idx=list(attack_idx), nlvr2_pair_pass=pair, **res)
        self.engine = FakeEngine(trace, pgd_dtype=L.F32 if pgd_f32 else None)
        self.trace, self.training, self.image_view, self.text_view = trace, training, image_view, text_view
        self.adv_lr, self.per_step_bs, self.augmentation = 0.005, B, False
        self.hparams = SimpleNamespace(config=cfg)
        self.grad_anchor = torch.zeros(1, requires_grad=True)
        pgd = {"moco": PA.PGDAttack_moco, "bt": PA.PGDAttack_bartlowtwins, "vqa": PA.PGDAttack_vqa, "nlvr2": PA.PGDAttack_nlvr2}[task]
        txt = {"moco": GA.GreedyAttack_moco, "bt": GA.GreedyAttack_barlowtwins, "vqa": GA.GreedyAttack_vqa, "nlvr2": GA.GreedyAttack_nlvr2}[task]
        self.pgd_attacker, self.greedy_attacker = pgd(cfg), txt(cfg)

    def grad_prescale(self):
        return 1.0

    def after_backward(self, overlap=False):
        self.trace.append(f"after_backward(overlap={overlap})")

    def log(self, key, value):
        self.trace.append(f"log({key})")


# ---- the scenarios ---------------------------------------------------------------------------------------------------------------------
def _batch(task):
    tok = WS.load_tokenizer(os.path.join(GOLDEN, "toy_vocab.txt"))
    ids, masks = WS.encode_sentences(tok, SENTENCES, LT)
    img = lambda: [torch.zeros(B, 3, S, S)]
    b = {"text": list(SENTENCES), "text_ids": ids, "text_masks": masks}
    if task == "nlvr2":
        b.update(image_0=img(), image_1=img(), answers=[True, False, True, True], table_name=["nlvr2_dev", "nlvr2_test1", "nlvr2_dev", "nlvr2_dev"])
    else:
        b["image"] = img()
    if task == "vqa":
        b.update(vqa_labels=[[1, 2], [], [3], [0, 4, 5]], vqa_scores=[[1.0, 0.3], [], [0.6], [1.0, 0.3, 0.3]])
    return b


def _objective(fn, task, grad=True, **kw):
    def run(trace):
        m = FakeModule(task, trace, **kw)
        with torch.set_grad_enabled(grad):
            ret = getattr(OBJ, fn)(m, _batch(task))
        trace.append("ret(" + ",".join(sorted(ret)) + ")")
        losses = [v for k, v in ret.items() if "loss" in k and torch.is_tensor(v) and v.requires_grad]
        if losses:
            trace.append("backward")
            sum(losses).backward()
    return run


def _keys(task):
    return torch.full((B, H3 if task == "bt" else PROJ), 0.5)


def _pgd_patches(task, hooks=False, clean_op=False, **kw):
    keep_prev = kw.pop("keep_prev", False)

    def run(trace):
        m = FakeModule(task, trace, **kw)
        eng, b = m.engine, _batch(task)
        pb = eng.bind_batch(b["text_ids"], b["text_masks"], b["image"][0], tag="t")
        extra = dict(clean_op=eng.make_operand(pb)) if clean_op else {}
        tgt = eng.vqa_targets(eng.vqa_bufs(B, "pgd"), b["vqa_labels"], b["vqa_scores"]) if task == "vqa" else _keys(task)
        if hooks:
            out = {}
            extra.update(before_first_loss=lambda: trace.append("before_first_loss"), clean_out=out)
        m.pgd_attacker.attack_patches(m, pb, tgt, keep_prev=keep_prev, **extra)
        if hooks:
            trace.append("clean_out(" + ",".join(sorted(out)) + ")")
    return run


def _pgd_public(task, **kw):
    def run(trace):
        m = FakeModule(task, trace, **kw)
        b = _batch(task)
        m.pgd_attacker.pgd_attack(m, b, k_modality=None if task in ("vqa", "nlvr2") else _keys(task))
    return run


def _greedy_parts(task, **kw):
    def run(trace):
        m = FakeModule(task, trace, **kw)
        att, eng, b = m.greedy_attacker, m.engine, _batch(task)
        ids, masks = b["text_ids"], b["text_masks"]
        att.calc_words_to_sub_words([s.split(" ") for s in SENTENCES], B)
        pb, op = att.bind_batch(m, b, ids, masks)
        de = torch.zeros(att.saliency_rows(pb) * LT, D)
        k = None if task in ("vqa", "nlvr2") else _keys(task)
        att.bind_keys(m, pb, k)
        att.set_text(pb, ids, masks)
        ctx, grads, _ = att.get_grad(m, pb, op, de)
        trace.append(f"grads{list(grads.shape)}")
        att.word_scores(m, pb, grads, B)
        owner = [0, 0, 1, 2, 2, 2, 3]
        n_real, Bc = len(owner), B * att.n_candidates
        own = torch.tensor(owner + [0] * (Bc - n_real))
        pc = att.bind_candidates(m, pb, op, own, ids.index_select(0, own).contiguous(), masks.index_select(0, own).contiguous())
        att.bind_candidate_keys(pc, k, own)
        picks = att.score(m, pc, ctx, owner, n_real, B)
        trace.append("picks(" + ",".join(str(j) for _, j in picks) + ")")
    return run


def _greedy_full(task, tokens=False, **kw):
    def run(trace):
        m = FakeModule(task, trace, **kw)
        att = m.greedy_attacker
        if tokens:
            att.tokenizer = None
        res = att.adv_attack_samples(m, _batch(task), None if task in ("vqa", "nlvr2") else _keys(task))
        trace.append("ids" + str(list(res["txt_input_ids"].shape)) + " changes" + str(res["changes_verification"]))
    return run


def scenarios():
    sc = {}
    for name, grad, train in (("train", True, True), ("nograd", False, True), ("eval", False, False)):
        sc[f"vqa/{name}"] = _objective("compute_vqa", "vqa", grad, training=train)
        for pair in (True, False):
            sc[f"nlvr2/{'pair' if pair else 'two_pass'}/{name}"] = _objective("compute_nlvr2", "nlvr2", grad, training=train, pair=pair)
    views = (("img", True, False), ("txt", False, True), ("both", True, True))
    for v, iv, tv in views:
        for K in (1, 2, 3):
            kw = dict(K=K, image_view=iv, text_view=tv)
            sc[f"vqa_attack/{v}/K{K}/train"] = _objective("compute_vqa_attack", "vqa", **kw)
            sc[f"bt/{v}/K{K}/train"] = _objective("compute_barlowtwins_contrastive", "bt", **kw)
            sc[f"nlvr2_attack/pair/{v}/idx11/K{K}/train"] = _objective("compute_nlvr2_attack", "nlvr2", **kw)
        kw = dict(K=2, image_view=iv, text_view=tv)
        for name, grad, train in (("nograd", False, True), ("eval", False, False)):
            sc[f"vqa_attack/{v}/K2/{name}"] = _objective("compute_vqa_attack", "vqa", grad, training=train, **kw)
            sc[f"bt/{v}/K2/{name}"] = _objective("compute_barlowtwins_contrastive", "bt", grad, training=train, **kw)
            sc[f"nlvr2_attack/pair/{v}/idx11/K2/{name}"] = _objective("compute_nlvr2_attack", "nlvr2", grad, training=train, **kw)
        for pair in (True, False):
            for idx in ((1, 1), (1, 0), (0, 1)):
                n = f"nlvr2_attack/{'pair' if pair else 'two_pass'}/{v}/idx{idx[0]}{idx[1]}/K2/train"
                sc.setdefault(n, _objective("compute_nlvr2_attack", "nlvr2", pair=pair, attack_idx=idx, **kw))
        sc[f"nlvr2_attack/two_pass/{v}/idx10/K2/eval"] = _objective("compute_nlvr2_attack", "nlvr2", False, training=False, pair=False,
                                                                     attack_idx=(1, 0), **kw)
    sc["vqa_attack/both/K2/train/pgd_f32"] = _objective("compute_vqa_attack", "vqa", K=2, image_view=True, text_view=True, pgd_f32=True)
    for task in ("moco", "bt", "vqa"):
        for K in (1, 2, 3):
            for keep in (False, True):
                for cop in (False, True):
                    sc[f"pgd/{task}/K{K}/keep{int(keep)}/clean_op{int(cop)}"] = _pgd_patches(task, K=K, keep_prev=keep, clean_op=cop)
        sc[f"pgd/{task}/K2/eval"] = _pgd_patches(task, K=2, training=False)
    for task in ("moco", "vqa"):                                   # (the loops that honour the engine's fp32 PGD twin)
        for cop in (False, True):
            sc[f"pgd/{task}/K2/pgd_f32/clean_op{int(cop)}"] = _pgd_patches(task, K=2, pgd_f32=True, keep_prev=True, clean_op=cop)
    for K in (1, 2, 3):
        sc[f"pgd/moco/K{K}/hooks"] = _pgd_patches("moco", hooks=True, K=K, clean_op=True)
    sc["pgd/moco/K2/hooks/pgd_f32"] = _pgd_patches("moco", hooks=True, K=2, pgd_f32=True)
    for task in ("moco", "bt", "vqa", "nlvr2"):
        for K in (1, 2, 3):
            sc[f"pgd_attack/{task}/K{K}"] = _pgd_public(task, K=K)
        sc[f"greedy/{task}/get_grad_score"] = _greedy_parts(task)
        sc[f"greedy/{task}/get_grad_score/eval"] = _greedy_parts(task, training=False)
        sc[f"greedy/{task}/adv_attack_samples"] = _greedy_full(task)
    for pair in (True, False):
        for idx in ((1, 1), (1, 0), (0, 1)):
            sc[f"pgd_attack/nlvr2/{'pair' if pair else 'two_pass'}/idx{idx[0]}{idx[1]}/K2"] = _pgd_public("nlvr2", K=2, pair=pair, attack_idx=idx)
        sc[f"greedy/nlvr2/{'pair' if pair else 'two_pass'}/get_grad_score"] = _greedy_parts("nlvr2", pair=pair)
        sc[f"greedy/nlvr2/{'pair' if pair else 'two_pass'}/adv_attack_samples"] = _greedy_full("nlvr2", pair=pair)
    for task in ("moco", "bt"):
        sc[f"greedy/{task}/adv_attack_samples/tokens"] = _greedy_full(task, tokens=True)
    return sc


# ---- recording -------------------------------------------------------------------------------------------------------------------------
class _Patched:
    """The delta-norm launch that is not an engine method in every form of the code (a direct library call with raw pointers) is
    written down as the engine method would be; ``stream_ptr`` needs no HIP stream here."""

    def __init__(self, trace_of):
        self.trace_of = trace_of

    def __enter__(self):
        self.saved = [(RT, "stream_ptr", RT.stream_ptr)] + [(mod, "stream_ptr", mod.stream_ptr) for mod in (OBJ, PA) if hasattr(mod, "stream_ptr")]
        for mod, n, _ in self.saved:
            setattr(mod, n, lambda: None)
        real = L.lib.rmcl_delta_channel_norm

        def norm(delta, out, *rest):
            eng = self.trace_of()
            eng.trace.append(f"delta_channel_norm({eng.name_ptr(delta.value)},{eng.name_ptr(out.value) or 'f32[1]'})")
            return 0

        self.saved.append((L.lib, "rmcl_delta_channel_norm", real))
        L.lib.rmcl_delta_channel_norm = norm
        return self

    def __exit__(self, *exc):
        for mod, n, v in self.saved:
            setattr(mod, n, v)


_LAST = []


def snapshot(only=None):
    out = {}
    real_init = FakeEngine.__init__

    def init(self, *a, **kw):
        real_init(self, *a, **kw)
        _LAST[:] = [self]

    FakeEngine.__init__ = init
    try:
        with _Patched(lambda: _LAST[0]):
            for name, run in scenarios().items():
                if only is None or name in only:
                    torch.manual_seed(0)
                    trace = []
                    run(trace)
                    out[name] = trace
    finally:
        FakeEngine.__init__ = real_init
    return out


def _digest(trace):
    return hashlib.sha256("\n".join(trace).encode()).hexdigest()


def _fixture(snap):
    return {name: dict({"n": len(t), "sha256": _digest(t)}, **({"calls": t} if name in FULL else {})) for name, t in snap.items()}


_SNAP = {}


def _snap():
    if not _SNAP:
        _SNAP.update(snapshot())
    return _SNAP


def test_every_scenario_is_recorded():
    want = json.load(open(FIXTURE))
    assert sorted(_snap()) == sorted(want) and all(n in want for n in FULL)


@pytest.mark.parametrize("name", FULL)
def test_call_list_equals_the_recorded_one(name):
    want, got = json.load(open(FIXTURE))[name]["calls"], _snap()[name]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: call {i} is {a}, recorded {b}"
    assert len(got) == len(want)


def test_call_digests_equal_the_recorded_ones():
    want = json.load(open(FIXTURE))
    bad = [(n, len(t), want[n]["n"]) for n, t in _snap().items() if (len(t), _digest(t)) != (want[n]["n"], want[n]["sha256"])]
    for n, _, _ in bad[:2]:                                    # (only digests are recorded for these: show what runs now)
        print(f"---- {n}: the engine calls now", *_snap()[n], sep="\n")
    assert not bad, f"{len(bad)} of {len(want)} scenarios differ from the recorded engine calls (name, calls now, calls recorded): {bad[:8]}"


if __name__ == "__main__":
    snap = snapshot()
    if "--record" in sys.argv:
        json.dump(_fixture(snap), open(FIXTURE, "w"), indent=0, sort_keys=True)
    if "--dump" in sys.argv:
        json.dump(snap, open(sys.argv[sys.argv.index("--dump") + 1], "w"), indent=0, sort_keys=True)
    print(len(snap), "scenarios,", sum(len(t) for t in snap.values()), "calls")
