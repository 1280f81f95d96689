"""Using a trained model: the predictions of the reference's ``demo.py`` (greedy ``[MASK]`` filling, word-patch alignment heat maps) and
``demo_vqa.py`` (the best VQA answer), and the ranked retrieval lists behind ``compute_irtr_recall`` - on the passes and head launchers
the training path already runs (``Engine.mlm_bind(all_rows=True)`` -> ``mlm_forward`` -> ``mlm_logits``, ``vqa_forward``, the cost chain
of compute_itm_wpa) plus one row kernel that the first three share, ``Engine.rows_topk`` (include/rmcl.h rmcl_rows_topk), and the two
alignment kernels ``Engine.ipot_plan`` / ``Engine.align_heat`` (rmcl_ipot_plan_f32, rmcl_align_heat).  DESIGN.md "Prediction API",
INTEGRATION.md "Predictions".

Every call runs under ``torch.no_grad()`` with the model in eval mode and puts the model's mode flags, the engine's dropout switch and
its pass counter back afterwards: a training step taken after a prediction is the step that would have been taken without it."""
from __future__ import annotations

import contextlib
import os

import torch

from . import _lib as L
from .attack.word_substitution import load_tokenizer
from .runtime import stream_ptr
from .task_loss import HEAD_ROWS


class Predictor:
    """``Predictor(model, tokenizer=None, id2answer=None)``.  tokenizer: a tokenizer object, or a local vocabulary (a ``vocab.txt`` or the
    directory holding one) - nothing is ever fetched, so a bare hub name is an error.  id2answer: label id -> answer string (a dict or a
    list); default: the model's own (``model.id2answer``, set by a VQA datamodule)."""

    def __init__(self, model, tokenizer=None, id2answer=None):
        self.model, self.eng = model, model.engine
        tok = load_tokenizer(tokenizer)
        if tokenizer is not None and tok is None:
            raise ValueError(f"tokenizer {os.fspath(tokenizer)!r} is neither a tokenizer object nor a local vocab.txt (or its directory): "
                             "nothing is fetched, so a hub name cannot be used here")
        self.tokenizer = tok
        self.id2answer = id2answer if id2answer is not None else getattr(model, "id2answer", None)

    # ---- the state a prediction borrows ------------------------------------------------------------------------------------
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

    # ---- inputs ------------------------------------------------------------------------------------------------------------
    def _max_len(self) -> int:
        return int(self.eng.cfg["max_text_len"])

    def _encode(self, text):
        """one tokenisation of a string or a list of strings: (ids [B, max_text_len], masks) on the host"""
        if self.tokenizer is None:
            raise ValueError("text input needs a tokenizer: Predictor(model, tokenizer=<object or local vocab.txt>), or pass text_ids / text_masks")
        text = [text] if isinstance(text, str) else list(text)
        enc = self.tokenizer(text, padding="max_length", truncation=True, max_length=self._max_len(), return_special_tokens_mask=False)
        return torch.tensor(enc["input_ids"], dtype=torch.int64), torch.tensor(enc["attention_mask"], dtype=torch.int64)

    def _text(self, text, text_ids, text_masks):
        if (text is None) == (text_ids is None):
            raise ValueError("give either text (a string or a list of strings) or text_ids (with text_masks), not both and not neither")
        if text is not None:
            return self._encode(text)
        ids = torch.as_tensor(text_ids)
        if ids.dim() == 1:
            ids = ids.view(1, -1)
        if ids.dim() != 2 or ids.shape[1] != self._max_len():
            raise ValueError(f"text_ids must be [B, max_text_len = {self._max_len()}] (got {tuple(ids.shape)}): pad to the model's text length")
        masks = torch.ones_like(ids) if text_masks is None else torch.as_tensor(text_masks).view(ids.shape)
        return ids.to(torch.int64), masks.to(torch.int64)

    @staticmethod
    def _image(image, B=None):
        if hasattr(image, "data") and hasattr(image, "sizes"):                  # a byte batch of the uint8 feed: bound as it is
            return image
        if not torch.is_tensor(image):
            raise ValueError("image must be a float tensor [3, H, W] or [B, 3, H, W] (or a uint8 batch of the byte feed)")
        img = image.unsqueeze(0) if image.dim() == 3 else image
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"image must be [3, H, W] or [B, 3, H, W] (got {tuple(image.shape)})")
        if B is not None and img.shape[0] != B:
            if img.shape[0] != 1:
                raise ValueError(f"{img.shape[0]} images for {B} texts")
            img = img.expand(B, -1, -1, -1)
        return img

    def _need(self, head: str, what: str):
        if getattr(self.eng, head) is None:
            raise ValueError(f"{what} needs a model built with loss_names[{head!r}] > 0 (the {head} head); this model has none")

    # ---- masked language modelling -----------------------------------------------------------------------------------------
    def _mlm_bind(self, B: int, N: int):
        """the all-rows buffers of a batch of B sentences, bound once: the labels are all ignored (-100, on the host: no read-back)"""
        labels = torch.full((B, self._max_len()), -100, dtype=torch.int64)
        return self.eng.mlm_bind(self.eng.mlm_bufs(B, "predict"), labels, N, all_rows=True)

    def _mlm_logits(self, pb, ma) -> torch.Tensor:
        """one MODE_INFER pass on the ids bound in `pb`, the all-rows MLM head, the dense logits [B * L, vocab]"""
        eng = self.eng
        op = eng.make_operand(pb, out=pb.patchesT_full)
        eng.encoder_forward(pb, key=False, mode=L.MODE_INFER, patchesT=op)
        eng.mlm_forward(ma, pb.xn)
        return eng.mlm_logits(ma, ma.M)

    def mlm_topk(self, batch, k: int = 5):
        """(ids [B, L, k] int64, probs [B, L, k]): the k most likely tokens of every text position of ``batch`` (``text_ids``,
        ``text_masks``, ``image``) with their softmax probabilities, most likely first; on the device."""
        self._need("mlm", "mlm_topk")
        eng = self.eng
        with self._eval():
            pb = eng.bind_batch(batch["text_ids"], batch["text_masks"], batch["image"][0], tag="predict")
            d = pb.d
            ma = self._mlm_bind(pb.B, d.L + 1 + d.P)
            idx, _, prob = eng.rows_topk(self._mlm_logits(pb, ma), k, "softmax")
            return idx.view(pb.B, d.L, k).to(torch.int64), prob.view(pb.B, d.L, k)

    def fill_mask(self, image, text=None, text_ids=None, text_masks=None, top_k: int = 5, mask_token_id: int = None):
        """The loop of the reference's demo.py on ids: every round, among the positions of a sentence that still hold the mask id, the one
        whose best token has the largest softmax probability (the first such position on a tie) takes that token; until no mask is left.
        A batch advances every sentence that has masks left by one position per round; a sentence without masks is returned unchanged.
        The ids stay on the device across the rounds and come back in one transfer at the end.

        Returns a dict: ``ids`` [B, L] (filled, on the host), ``text`` (list of decoded strings; with a tokenizer), ``fills``: per sentence
        the list of its fills in the order they were made, each ``{"position", "token_id", "prob", "top_ids", "top_probs"}`` (+ ``"token"``
        and ``"top_tokens"`` with a tokenizer).  mask_token_id: default ``tokenizer.mask_token_id``."""
        self._need("mlm", "fill_mask")
        if mask_token_id is None:
            if self.tokenizer is None:
                raise ValueError("fill_mask needs the mask id: Predictor(model, tokenizer=...) (tokenizer.mask_token_id) or mask_token_id=")
            mask_token_id = self.tokenizer.mask_token_id
        ids, masks = self._text(text, text_ids, text_masks)
        B, Lt = int(ids.shape[0]), int(ids.shape[1])
        if not 1 <= int(top_k) <= L.TOPK_MAX:
            raise ValueError(f"top_k must be in 1 .. {L.TOPK_MAX} (got {top_k})")
        eng = self.eng
        # the number of rounds: counted where the ids are - on the host for a tokenised text or host ids (no device read); ids handed
        # over on the device cost this one scalar
        rounds = int(((ids == mask_token_id) & (masks != 0)).sum(dim=1).max()) if B else 0
        with self._eval():
            pb = eng.bind_batch(ids, masks, self._image(image, B), tag="predict")
            dev_ids = pb.text_ids.clone() if pb.text_ids.data_ptr() == ids.data_ptr() else pb.text_ids     # (never the caller's tensor)
            pb.text_ids = dev_ids
            d = pb.d
            ma = self._mlm_bind(B, d.L + 1 + d.P) if rounds else None
            ar = torch.arange(B, device=eng.device)
            rec = []
            for _ in range(rounds):
                idx, _, prob = eng.rows_topk(self._mlm_logits(pb, ma), top_k, "softmax")
                idx, prob = idx.view(B, Lt, top_k), prob.view(B, Lt, top_k)
                live = (dev_ids == mask_token_id) & (pb.text_mask != 0)
                score = torch.where(live, prob[:, :, 0], torch.full_like(prob[:, :, 0], -1.0)).contiguous()
                pos = eng.rows_topk(score, 1)[0].view(B).to(torch.int64)       # the first maximum: the kernel's tie rule, not torch's
                has = live.any(dim=1)
                tok = idx[ar, pos].to(torch.int64)                             # [B, top_k]
                dev_ids[ar, pos] = torch.where(has, tok[:, 0], dev_ids[ar, pos])
                rec.append(torch.cat([has.to(torch.int64).view(B, 1), pos.view(B, 1), tok,
                                      prob[ar, pos].contiguous().view(torch.int32).to(torch.int64)], dim=1))
            packed = torch.cat([dev_ids] + rec, dim=1).cpu()                   # the one read-back
        out_ids = packed[:, :Lt].contiguous()
        fills = [[] for _ in range(B)]
        w = 2 + 2 * top_k
        for r in range(rounds):
            blk = packed[:, Lt + r * w: Lt + (r + 1) * w]
            for b in range(B):
                if int(blk[b, 0]):
                    t_ids = blk[b, 2: 2 + top_k].tolist()
                    t_pr = blk[b, 2 + top_k:].to(torch.int32).view(torch.float32).tolist()
                    f = {"position": int(blk[b, 1]), "token_id": t_ids[0], "prob": t_pr[0], "top_ids": t_ids, "top_probs": t_pr}
                    if self.tokenizer is not None:
                        f["top_tokens"] = self.tokenizer.convert_ids_to_tokens(t_ids)
                        f["token"] = f["top_tokens"][0]
                    fills[b].append(f)
        ret = {"ids": out_ids, "fills": fills}
        if self.tokenizer is not None:
            keep = masks.cpu().bool()                                          # (a no-op for host masks)
            ret["text"] = [self.tokenizer.decode(row[m].tolist(), skip_special_tokens=True) for row, m in zip(out_ids, keep)]
        return ret

    # ---- VQA ---------------------------------------------------------------------------------------------------------------
    def answer(self, batch, top_k: int = 1):
        """The VQA answers of a batch dict (``text_ids``, ``text_masks``, ``image``) or of ``(image, question)`` (a string or a list of
        strings; needs the tokenizer): a dict with ``ids`` [B, k] int64, ``logits`` [B, k], ``scores`` [B, k] = sigmoid(logits), best
        first, on the device, and ``answers`` (lists of strings) when id2answer is known.  ``ids[:, 0]`` is ``vqa_preds`` of compute_vqa /
        test_step: the first maximum of the logits."""
        self._need("vqa", "answer")
        eng = self.eng
        if isinstance(batch, dict):
            ids, masks, image = batch["text_ids"], batch["text_masks"], batch["image"][0]
        else:
            image, question = batch
            ids, masks = self._encode(question)
            image = self._image(image, int(ids.shape[0]))
        N = int(eng.vqa.N)
        if not 1 <= int(top_k) <= min(N, L.TOPK_MAX):
            raise ValueError(f"top_k must be in 1 .. {min(N, L.TOPK_MAX)} (got {top_k})")
        with self._eval():
            pb = eng.bind_batch(ids, masks, image, tag="predict")
            op = eng.make_operand(pb, out=pb.patchesT_full)
            eng.encoder_forward(pb, key=False, mode=L.MODE_INFER, patchesT=op, cls_tail=True)
            eng.heads_forward(pb, key=False, want_q=False, wgrad=False)
            B = pb.B
            out_i = torch.empty(B, top_k, dtype=torch.int64, device=eng.device)
            out_z = torch.empty(B, top_k, dtype=torch.float32, device=eng.device)
            out_p = torch.empty(B, top_k, dtype=torch.float32, device=eng.device)
            for s in range(0, B, HEAD_ROWS):                                   # the head launcher takes at most 256 rows
                e = min(B, s + HEAD_ROWS)
                vb = eng.vqa_bufs(e - s, "predict")
                i, z, p = eng.rows_topk(eng.vqa_forward(vb, pb.cls[s:e]), top_k, "sigmoid")      # (the [n, N] view of the pitched logits)
                out_i[s:e], out_z[s:e], out_p[s:e] = i, z, p
        ret = {"ids": out_i, "logits": out_z, "scores": out_p}
        if self.id2answer is not None:
            ret["answers"] = [[self.id2answer[int(a)] for a in row] for row in out_i.tolist()]
        return ret

    # ---- word-patch alignment ----------------------------------------------------------------------------------------------
    def align(self, image, text=None, text_ids=None, text_masks=None, token=None, iterations: int = 1000, beta: float = 0.1, size=None):
        """Where the words of a sentence land on the image: the heat maps of the reference's demo.py:86-151.  One MODE_INFER pass, the
        demo's masks (``[CLS]``, the last valid text token and the image cls slot are dropped), the masked cosine cost of compute_itm_wpa
        on the normalised features, the transport plan of ``ipot(cost, ..., beta, iterations, k = 1)`` (``Engine.ipot_plan``), and per text
        position its plan column scattered to the patch grid, standardised, clipped to [1, 3] sigma and min-max normalised
        (``Engine.align_heat``).  Needs no head.

        Returns a dict, tensors on the device: ``plan`` [B, Li, Lt]; ``cost`` [B, Lt, Li] (the masked cosine cost behind it); ``grid`` / ``heat`` [B, Lt, H, W]; ``flat`` [B, Lt] int32 - 1 where
        the demo's arithmetic divides by zero (a position the masks drop, or a map whose clipped values are all equal): ``heat`` is 0
        there, not NaN; ``grid_hw`` = (H, W); ``tokens`` (per sample the token strings; with a tokenizer); and with ``token`` (a text
        position, or one per sample) ``alpha`` [B, Hout, Wout] uint8: ``uint8(heat * 255)`` of that position enlarged like PIL's NEAREST
        to ``size`` = (height, width), default the pixel extent of the bound image batch."""
        ids, masks = self._text(text, text_ids, text_masks)
        B, Lt = int(ids.shape[0]), int(ids.shape[1])
        iterations, beta = int(iterations), float(beta)
        if not 1 <= iterations <= L.IPOT_PLAN_MAX_ITERS:
            raise ValueError(f"iterations must be in 1 .. {L.IPOT_PLAN_MAX_ITERS} (got {iterations})")
        if not beta > 0.0:
            raise ValueError(f"beta must be > 0 (got {beta})")
        if Lt > L.IPOT_PLAN_MAX_LT:
            raise ValueError(f"align takes a max_text_len of at most {L.IPOT_PLAN_MAX_LT} (this model: {Lt})")
        if token is not None:
            token = [int(token)] * B if isinstance(token, int) else [int(v) for v in token]
            if len(token) != B or any(not 0 <= v < Lt for v in token):
                raise ValueError(f"token must be a text position in 0 .. {Lt - 1}, or one per sample ({B} samples; got {token})")
        if size is not None and not (len(size) == 2 and all(1 <= int(v) <= 16384 for v in size)):
            raise ValueError(f"size must be (height, width) with both in 1 .. 16384 (got {size})")
        eng = self.eng
        with self._eval():
            pb = eng.bind_batch(ids, masks, self._image(image, B), tag="predict")
            d = pb.d
            Li, D = d.P + 1, d.D
            N = Lt + Li
            if Li > L.IPOT_PLAN_MAX_LI:
                raise ValueError(f"align takes at most {L.IPOT_PLAN_MAX_LI - 1} image patches (this batch: {d.P})")
            op = eng.make_operand(pb, out=pb.patchesT_full)
            eng.encoder_forward(pb, key=False, mode=L.MODE_INFER, patchesT=op)
            dev = eng.device
            # masks (demo.py:97-105): drop [CLS], the last valid text token and the image cls slot
            txt_mask = pb.text_mask.bool().clone()
            lens = txt_mask.sum(dim=1)
            txt_mask[torch.arange(B, device=dev), lens - 1] = False
            txt_mask[:, 0] = False
            img_mask = pb.co_mask[:, Lt:].bool().clone()
            img_mask[:, 0] = False
            txt_valid, img_valid = txt_mask.to(torch.int32).contiguous(), img_mask.to(torch.int32).contiguous()
            # the cost chain of compute_itm_wpa (vilt/modules/objectives.py), launch for launch
            st = stream_ptr()
            ld, M = (Li + 3) // 4 * 4, B * N
            xhat, norms = torch.empty(M, D, device=dev), torch.empty(M, device=dev)
            L.check(L.lib.rmcl_l2norm_rows_fwd(L.P(pb.xn), L.P(xhat), L.P(norms), M, D, L.F(1e-5), st), "l2norm")
            cost = torch.zeros(B, Lt, ld, device=dev)
            L.check(L.lib.rmcl_gemm_batched(L.P(xhat), L.P(xhat[Lt:]), L.P(cost), Lt, Li, D, L.I64(D), L.I64(D), ld, L.F(1.0), B, L.I64(N * D),
                                            L.I64(N * D), L.I64(Lt * ld), L.F32, L.F32, 1, 1, st), "cosine sim")
            L.check(L.lib.rmcl_wpa_cost_finish(L.P(cost), L.P(txt_valid), L.P(img_valid), B, Lt, Li, ld, st), "cost_finish")
            plan = eng.ipot_plan(cost, txt_valid, img_valid, beta, iterations)
            # the grid cell of every image slot, as infer builds patch_index (vilt_module.py:462-470)
            geom = pb.geom
            if geom is None:
                gh = gw = int(eng.cfg["image_size"]) // int(eng.cfg["patch_size"])
                pidx = torch.arange(gh * gw, dtype=torch.int32, device=dev).repeat(B, 1)
                extent = (int(eng.cfg["image_size"]),) * 2
            else:
                gh, gw = int(geom.gh), int(geom.gw)
                kept = torch.arange(d.P, device=dev)[None, :] < geom.counts[:, None]
                pidx = torch.where(kept, geom.sel[:, :d.P], torch.full_like(geom.sel[:, :d.P], -1))
                extent = (int(geom.shape[2]), int(geom.shape[3]))
            grid, heat, flat, alpha = eng.align_heat(plan, pidx.contiguous(), txt_valid, (gh, gw), token,
                                                     (extent if size is None else size) if token is not None else None)
        ret = {"plan": plan, "grid": grid, "heat": heat, "flat": flat, "grid_hw": (gh, gw), "cost": cost[:, :, :Li]}
        if alpha is not None:
            ret["alpha"] = alpha
        if self.tokenizer is not None:
            ret["tokens"] = [self.tokenizer.convert_ids_to_tokens(row) for row in ids.tolist()]
        return ret

    # ---- retrieval ---------------------------------------------------------------------------------------------------------
    def retrieve(self, scores: torch.Tensor, iids: torch.Tensor, tiids: torch.Tensor, k: int = 10):
        """Ranked lists of a score matrix [images, captions] (``compute_irtr_recall(return_scores=True)``; iids: the image ids of the rows,
        tiids: the image id of every caption).  Per image its k best captions - ``captions`` [I, k] (columns), ``caption_scores``,
        ``caption_iids`` (tiids of those columns) - and per caption its k best images - ``images`` [T, k] (rows), ``image_scores``,
        ``image_iids``; best first, ties to the smaller index, on the device.  The caption direction runs on a transposed contiguous copy."""
        eng = self.eng
        if not torch.is_tensor(scores) or scores.dim() != 2:
            raise ValueError("scores must be a 2-D tensor [images, captions]")
        iids, tiids = torch.as_tensor(iids).view(-1), torch.as_tensor(tiids).view(-1)
        if tuple(scores.shape) != (iids.numel(), tiids.numel()):
            raise ValueError(f"scores must be [images, captions] = [{iids.numel()}, {tiids.numel()}] (got {tuple(scores.shape)})")
        if not 1 <= int(k) <= min(min(scores.shape), L.TOPK_MAX):
            raise ValueError(f"k must be in 1 .. min(images, captions, {L.TOPK_MAX}) (got {k} for {tuple(scores.shape)})")
        s = scores.to(eng.device, torch.float32)
        s = s if s.stride(1) == 1 else s.contiguous()
        iids, tiids = iids.to(eng.device), tiids.to(eng.device)
        cap, cap_s, _ = eng.rows_topk(s, k)
        img, img_s, _ = eng.rows_topk(s.t().contiguous(), k)
        cap, img = cap.to(torch.int64), img.to(torch.int64)
        # (a slot a row of NaNs could not fill holds -1: its id is -1 too)
        ids_of = lambda table, idx: torch.where(idx >= 0, table[idx.clamp_min(0)], torch.full_like(idx, -1).to(table.dtype))
        return {"captions": cap, "caption_scores": cap_s, "caption_iids": ids_of(tiids, cap),
                "images": img, "image_scores": img_s, "image_iids": ids_of(iids, img)}

    def recall(self, scores: torch.Tensor, iids: torch.Tensor, tiids: torch.Tensor):
        """(ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10) from the ranked lists: what ``irtr_recall_from_scores`` returns."""
        if min(scores.shape) < 10:
            raise ValueError(f"R@10 needs at least 10 images and 10 captions (got {tuple(scores.shape)})")
        r = self.retrieve(scores, iids, tiids, k=10)
        iids, tiids = torch.as_tensor(iids).view(-1).to(self.eng.device), torch.as_tensor(tiids).view(-1).to(self.eng.device)
        hit_t = r["caption_iids"] == iids.view(-1, 1)              # [I, 10]: the caption at rank j belongs to the image
        hit_i = r["image_iids"] == tiids.view(-1, 1)               # [T, 10]: the image at rank j is the caption's
        # hits / n divided once, on the host: fp32 scalars with the bits of irtr_recall_from_scores
        share = lambda hit, kk: torch.tensor(int(hit[:, :kk].any(dim=1).sum()) / hit.shape[0], dtype=torch.float32)
        return (share(hit_i, 1), share(hit_i, 5), share(hit_i, 10), share(hit_t, 1), share(hit_t, 5), share(hit_t, 10))
