"""``ViLTransformerSS``: the reference's LightningModule API (vilt/modules/vilt_module.py:20-507) over
the MI355X engine.  Same constructor keys, state-dict names, ``infer`` / ``infer_k`` / ``forward`` /
``training_step`` / ``configure_optimizers``; pytorch_lightning is not required (plain nn.Module with a
minimal ``log`` / ``hparams`` shim), the caller may be any loop that does
``loss = m.training_step(batch, i); loss.backward(); opt.step()``."""
from __future__ import annotations

import ctypes as C
import math
import os
import types

import torch
import torch.nn as nn

from ... import _lib as L
from ..._lib import lib, check
from ...runtime import Engine, EMA_GROUPS
from ...attack.pgd_attack_vilt import PGDAttack_moco, PGDAttack_bartlowtwins, PGDAttack_vqa, PGDAttack_nlvr2
from ...attack.greedy_attack_vilt import GreedyAttack_moco, GreedyAttack_barlowtwins, GreedyAttack_vqa, GreedyAttack_nlvr2
from . import objectives, vilt_utils, dist_utils


def config_patch(module) -> int:
    return int(module.hparams.config["patch_size"])


class _Node(nn.Module):
    """anonymous container so parameters get the reference's dotted state-dict names"""


def _attach(root: nn.Module, dotted: str, param: nn.Parameter):
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Node())
        mod = mod._modules[p]
    mod.register_parameter(parts[-1], param)


class _InferFeatures(torch.autograd.Function):
    """The four feature tensors of ``infer`` with a backward: their gradients are handed to the closure, which launches the HIP
    heads / encoder backward into the gradient arena (every ``param.grad`` is a view of it)."""

    @staticmethod
    def forward(ctx, anchor, closure, prescale, text_feats, image_feats, cls_feats, raw_cls_feats):
        ctx.closure, ctx.prescale = closure, float(prescale)
        return text_feats.clone(), image_feats.clone(), cls_feats.clone(), raw_cls_feats.clone()

    @staticmethod
    def backward(ctx, g_txt, g_img, g_cls, g_raw):
        sc = (lambda g: None if g is None else (g * ctx.prescale if ctx.prescale != 1.0 else g))
        ctx.closure(sc(g_txt), sc(g_img), sc(g_cls), sc(g_raw))
        return None, None, None, None, None, None, None


class _SlotClosure:
    """The backward closure of one differentiable ``infer`` call together with its stash slot: the slot becomes free again when the
    backward has run or when autograd drops the graph (the closure is garbage-collected with the autograd node)."""

    def __init__(self, fn, busy: set, slot: int):
        self.fn, self.busy, self.slot = fn, busy, slot

    def __call__(self, *grads):
        try:
            self.fn(*grads)
        finally:
            self.busy.discard(self.slot)

    def __del__(self):
        self.busy.discard(self.slot)


class ViLTransformerSS(nn.Module):
    MAX_PENDING_INFER = 4

    def __init__(self, config, device="cuda:0", compute_dtype="bf16", exact=False, pgd_dtype=None):
        super().__init__()
        self.hparams = types.SimpleNamespace(config=config)
        self.config = config
        if config["loss_names"].get("irtr_attacked", 0) > 0:
            # PGDAttack_irtr.pgd_attack reads the undefined name `text_representation` (pgd_attack_vilt.py:391): the reference has no
            # arithmetic an attacked IRTR step (or compute_attacked_irtr_recall / GreedyAttack_irtr) could be pinned to
            raise NotImplementedError("loss_names['irtr_attacked'] > 0: the reference's PGDAttack_irtr.pgd_attack reads the undefined name "
                                      "`text_representation` (attack/pgd_attack_vilt.py:391), so there is nothing to reproduce; use loss_names['irtr']")
        if config["loss_names"].get("mpp", 0) > 0 and (config["loss_names"].get("moco", 0) > 0 or config["loss_names"].get("barlowtwins", 0) > 0):
            # the reference names no such recipe; a momentum copy of transformer.mask_token is not built
            raise NotImplementedError("loss_names['mpp'] > 0 together with 'moco' or 'barlowtwins' is not built (no reference recipe combines them)")
        self.engine = Engine(config, device, compute_dtype, exact, pgd_dtype)
        eng = self.engine
        if config.get("ln_fold") is False:
            eng.fold = {}
        self.current_tasks = []
        self.logged = {}
        self.epoch_metrics = None          # the epoch-metric table (vilt_utils.set_metrics); None: the objectives queue nothing
        self._infer_busy = set()               # stash slots of differentiable infer() calls whose backward is pending
        # query parameters = views into the flat fp32 arena; .grad = views into the gradient arena
        for name, off, shape in eng.specs:
            if name.startswith("itm_score") and config["loss_names"].get("itm", 0) <= 0:
                continue
            if name.startswith("moco_head") and config["loss_names"].get("moco", 0) <= 0:
                continue
            if name.startswith("itm_score") and eng.irtr:
                # vilt_module.py:237-239: the ITM head is frozen in an IRTR model (its row 1 still moves: rank_output below IS that row)
                _attach(self, name, nn.Parameter(eng.view(eng.q32, off, shape), requires_grad=False))
                continue
            p = nn.Parameter(eng.view(eng.q32, off, shape))
            p.grad = eng.view(eng.g32, off, shape)
            _attach(self, name, p)
        for name, off, shape in eng.alias_specs:
            # rank_output = Linear(D, 1) whose weight / bias are VIEWS of row 1 of itm_score.fc (vilt_module.py:233-236): same storage, so
            # an optimizer step on rank_output moves itm_score.fc.weight[1] and the state dict holds both
            if config["loss_names"].get("itm", 0) <= 0:
                raise ValueError("loss_names['irtr'] > 0 needs loss_names['itm'] > 0: rank_output is row 1 of itm_score.fc (vilt_module.py:233-236)")
            p = nn.Parameter(eng.view(eng.q32, off, shape))
            p.grad = eng.view(eng.g32, off, shape)
            _attach(self, name, p)
        self.transformer.visual_embed = self.visual_embed                # the reference's pl_module.transformer.visual_embed
        self.init_weights()
        if config["loss_names"].get("moco", 0) > 0:
            self.multimodal = config.get("Multimodal", True)
            self.per_step_bs = config["num_gpus"] * config["num_nodes"] * config["per_gpu_batchsize"]
            for name, off, shape in eng.specs:
                if name.split(".")[0] in EMA_GROUPS:
                    p = nn.Parameter(eng.view(eng.k32, off, shape), requires_grad=False)
                    _attach(self, "k_" + name, p)
            self.shadow_momentum_encoder()
            self.momentum = config["momentum"]
            self.temperature = config["temperature"]
            self.text_view = config["text_view"]
            self.augmentation = config["augmentation"]
            self.image_view = config["image_view"]
            self.num_negative = config["num_negative"]
            self.register_buffer("proj_queue", torch.randn(128, self.num_negative, device=eng.device))
            self.register_buffer("proj_queue_ptr", torch.zeros(1, dtype=torch.long, device=eng.device))
            eng.queue = self.proj_queue
            self._queue_ptr_host = 0
            if self.image_view and not self.augmentation:
                self.pgd_attacker = PGDAttack_moco(config)
            if self.text_view and not self.augmentation:
                self.greedy_attacker = GreedyAttack_moco(config)
        if config["loss_names"].get("barlowtwins", 0) > 0:                 # vilt_module.py:109-131
            self.multimodal = config.get("Multimodal", True)
            self.per_step_bs = config["num_gpus"] * config["num_nodes"] * config["per_gpu_batchsize"]
            self.text_view = config["text_view"]
            self.image_view = config["image_view"]
            self.augmentation = config["augmentation"]
            self.adv_lr = config["adv_lr"]
            self.loss_weight = 0.001
            H = eng.bt
            o = 0
            for i, (key, n) in enumerate((("projector.1", H.H1), ("projector.4", H.H2), ("norm", H.H3))):
                node = self                                               # nn.BatchNorm1d buffers under the reference's names
                for part in ("barlowtwins_head." + key).split("."):
                    if part not in node._modules:
                        node.add_module(part, _Node())
                    node = node._modules[part]
                node.register_buffer("running_mean", eng.bt_running[o:o + n])
                node.register_buffer("running_var", eng.bt_running[o + n:o + 2 * n])
                node.register_buffer("num_batches_tracked", eng.bt_tracked[i])
                o += 2 * n
            if self.text_view and not self.augmentation:
                self.greedy_attacker = GreedyAttack_barlowtwins(config)
            if self.image_view and not self.augmentation:
                self.pgd_attacker = PGDAttack_bartlowtwins(config)
        ln = config["loss_names"]
        if ln.get("vqa_attacked", 0) > 0:                                  # vilt_module.py:175-191
            self.image_view = config.get("image_view", False)
            self.text_view = config.get("text_view", False)
            if not (self.image_view or self.text_view):
                # the reference reaches compute_vqa_attack with `infer` unbound (NameError, objectives.py:825) - this default of
                # task_finetune_vqa_randaug_attacked is refused here, at construction
                raise ValueError("loss_names['vqa_attacked'] > 0 needs image_view=True and / or text_view=True")
            if self.text_view:
                # word level only: NotImplementedError unless config["tokenizer"] is a tokenizer object / a local vocabulary
                self.greedy_attacker = GreedyAttack_vqa(config)
            if self.image_view:
                self.pgd_attacker = PGDAttack_vqa(config)
        if ln.get("nlvr2_attacked", 0) > 0:                                # vilt_module.py:211-231
            self.image_view = config.get("image_view", False)
            self.text_view = config.get("text_view", False)
            if not (self.image_view or self.text_view):
                # the reference returns no nlvr2_attacked_loss then and its logging raises a KeyError (defect (b))
                raise ValueError("loss_names['nlvr2_attacked'] > 0 needs image_view=True and / or text_view=True")
            if self.text_view:
                # word level only: NotImplementedError unless config["tokenizer"] is a tokenizer object / a local vocabulary
                self.greedy_attacker = GreedyAttack_nlvr2(config)
            self.attack_idx = [bool(a) for a in config.get("attack_idx", [False, False])]   # (reference default: config.py:92)
            if self.image_view:
                if len(self.attack_idx) != 2 or not any(self.attack_idx):
                    # compute_pgd divides the delta log by sum(attack_idx) (objectives.py:183): [False, False] is a division by zero (defect (c))
                    raise ValueError(f"nlvr2_attacked with image_view needs attack_idx with at least one True of two (got {config.get('attack_idx')})")
                self.pgd_attacker = PGDAttack_nlvr2(config)
        self.id2answer = None                      # answer strings of the label ids (test_step); the reference reads them from its datamodule
        self.grad_anchor = torch.zeros((), device=eng.device, requires_grad=True)
        self.sync_grads = True                     # False on the early micro-steps of gradient accumulation (DDP no_sync)
        self.step_sync = dist_utils.StepGradSync(algo=config.get("grad_allreduce_algo", "ring"), compress=config.get("grad_allreduce_dtype"))
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._after_load())
        # downstream checkpoint (vilt_module.py:134-160, test_only twin :252-268): loaded AFTER the momentum copies were
        # shadowed, strict=False, like the reference - so k_* keys absent from the file keep their pre-load values
        if config.get("load_path", "") not in ("", None):
            self._load_checkpoint(config["load_path"])

    def _load_checkpoint(self, path):
        # weights_only=True: executes nothing from the file (the reference uses a full unpickle, vilt_module.py:138)
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        state_dict = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
        if self.hparams.config["loss_names"].get("mlm", 0) > 0 and not self.hparams.config.get("test_only", False):
            # MLM head from the 200k checkpoint when that file exists (:140-150; the reference fails without it, here the head of the
            # loaded file - or the initialisation - stays)
            for cand in ("models_weight/vilt_200k_mlm_itm.ckpt", "../models_weight/vilt_200k_mlm_itm.ckpt"):
                if os.path.isfile(cand):
                    c2 = torch.load(cand, map_location="cpu", weights_only=True)["state_dict"]
                    for k in ("mlm_score.bias", "mlm_score.transform.dense.weight", "mlm_score.transform.dense.bias",
                              "mlm_score.transform.LayerNorm.weight", "mlm_score.transform.LayerNorm.bias", "mlm_score.decoder.weight"):
                        state_dict[k] = c2[k]
                    break
        if self.hparams.config["loss_names"].get("itm", 0) > 0:          # ITM head from the 200k checkpoint (:152-159)
            for cand in ("models_weight/vilt_200k_mlm_itm.ckpt", "../models_weight/vilt_200k_mlm_itm.ckpt"):
                if os.path.isfile(cand):
                    c2 = torch.load(cand, map_location="cpu", weights_only=True)["state_dict"]
                    state_dict["itm_score.fc.weight"] = c2["itm_score.fc.weight"]
                    state_dict["itm_score.fc.bias"] = c2["itm_score.fc.bias"]
                    break
        mine = self.state_dict()
        nl3 = self.engine.nlvr2 is not None and not self.hparams.config.get("test_only", False)
        if nl3:
            # NLVR2 (vilt_module.py:134-160 then :193-231): the training-time load fills the PRE-resize 2-row table; the resize then keeps
            # rows 0 / 1 and copies row 1 into row 2.  A 3-row table in that position is a size mismatch, as in the reference
            mine = dict(mine)
            mine["token_type_embeddings.weight"] = mine["token_type_embeddings.weight"][:2]
        # a tensor of another shape (position table at another resolution, text positions at another max_text_len) is an ERROR like
        # in the reference, whose load_state_dict(strict=False) raises on size mismatches (vilt_module.py:159-160) - not a silent skip
        wrong = [(k, tuple(v.shape), tuple(mine[k].shape)) for k, v in state_dict.items() if k in mine and tuple(mine[k].shape) != tuple(v.shape)]
        if wrong:
            raise RuntimeError("Error(s) in loading state_dict: " + "; ".join(f"size mismatch for {k}: checkpoint {a}, model {b}" for k, a, b in wrong))
        # downstream heads exist only AFTER the training-time load in the reference (vilt_module.py:134-160 loads, :164 builds the VQA
        # head): a checkpoint's vqa_classifier.* keep their init unless test_only (:254-268 loads after the heads were built)
        # rank_output likewise (:233-236, built after the load as a view of the loaded itm_score row 1); under test_only the file's own
        # rank_output.* load after itm_score.* (module order), so they win on row 1
        late = () if self.hparams.config.get("test_only", False) else ("vqa_classifier.", "nlvr2_classifier.", "rank_output.")
        take = {k: v for k, v in state_dict.items() if k in mine and not k.startswith(late)}
        tt = take.pop("token_type_embeddings.weight", None) if nl3 else None
        res = self.load_state_dict(take, strict=False)
        if nl3:
            with torch.no_grad():
                w = dict(self.named_parameters())["token_type_embeddings.weight"]
                if tt is not None:
                    w[:2].copy_(tt)
                w[2].copy_(w[1])                                        # rows [0, 1, 1] (vilt_module.py:202-205)
                self.engine.lp_stale = True
        unexpected = sorted(k for k in state_dict if k not in take)
        self.load_report = {"missing": sorted(res.missing_keys), "unexpected": unexpected}
        if res.missing_keys or unexpected:
            import warnings
            warnings.warn(f"load_path={path}: {len(res.missing_keys)} model tensors not in the checkpoint (kept: "
                          f"{', '.join(sorted(res.missing_keys)[:6])}{' ...' if len(res.missing_keys) > 6 else ''}); "
                          f"{len(unexpected)} checkpoint tensors unused ({', '.join(unexpected[:6])}{' ...' if len(unexpected) > 6 else ''})")
        # LayerNorm fold after a checkpoint load.  Round 3 switched it off here: the folded GEMM ate bf16(x) of the RAW residual stream,
        # whose rounding grows with the row's common-mode offset (a trained checkpoint's stream is not zero-mean).  Since round 4 the
        # producers store bf16(x - c) with c = the row mean of the row's previous LayerNorm (LN(x) = LN(x - c) exactly; gemm.h
        # ln_center), so the operand's rounding follows the row's spread whatever its offset (tests/test_kernels_gpu.py
        # test_layernorm_fold_precision_on_offset_rows: fold within 2x of the separate LayerNorm at 10 and 50 sigma) and the fold STAYS
        # ON.  config["ln_fold"] = False switches it off (separate LayerNorm kernels in every pass).
        self.load_report["ln_fold"] = "on (shift-robust form)" if self.engine.fold else "off"
        return res

    # ---- initialisation (objectives.init_weights :1505-1516, ViT _init_weights :512-519) ----
    @torch.no_grad()
    def init_weights(self):
        for name, p in self.named_parameters():
            if name.startswith("k_"):
                continue
            leaf = name.split(".")[-1]
            is_ln = any(t in name for t in ("LayerNorm", "norm1", "norm2", "transformer.norm", "projector.1"))
            if name == "transformer.mask_token":
                p.zero_()                         # VisionTransformer.__init__ leaves nn.Parameter(torch.zeros(1, 1, D)) as it is
            elif name.startswith(("vqa_classifier.", "nlvr2_classifier.")):
                # objectives.init_weights (:1505-1516) applied to the head (vilt_module.py:172, :200): Linear N(0, 0.02) / bias 0, LayerNorm
                # 1 / 0 (the substring rule below would miss the LayerNorm gain "vqa_classifier.1.weight")
                if name.startswith(("vqa_classifier.1.", "nlvr2_classifier.1.")):
                    p.fill_(1.0 if leaf == "weight" else 0.0)
                elif leaf == "bias":
                    p.zero_()
                else:
                    p.normal_(mean=0.0, std=0.02)
            elif name.startswith("barlowtwins_head."):
                # never passed through init_weights in the reference (vilt_module.py:115): nn.Linear / nn.BatchNorm1d defaults
                if p.dim() == 2:
                    nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                else:
                    p.fill_(1.0 if leaf == "weight" else 0.0)
            elif is_ln:
                p.fill_(1.0 if leaf == "weight" else 0.0)
            elif name.startswith("transformer.patch_embed.proj"):
                # the reference leaves the patch projection at nn.Conv2d's default init (vision_transformer.py:397-403;
                # VisionTransformer._init_weights :512-519 only touches nn.Linear / nn.LayerNorm)
                fan_in = p.shape[1] * p.shape[2] * p.shape[3] if p.dim() == 4 else 3 * config_patch(self) ** 2
                if leaf == "weight":
                    nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                else:
                    bound = 1.0 / math.sqrt(fan_in)
                    p.uniform_(-bound, bound)
            elif leaf == "bias":
                p.zero_()
            elif name.startswith("transformer."):
                nn.init.trunc_normal_(p, std=0.02)
            else:
                p.normal_(mean=0.0, std=0.02)
            if name == "token_type_embeddings.weight" and p.shape[0] == 3:
                p[2].copy_(p[1])                  # NLVR2: Embedding(3, D) with rows [old0, old1, old1] (vilt_module.py:201-205)
        self.engine.lp_stale = True

    @torch.no_grad()
    def shadow_momentum_encoder(self):
        """_shadow_layer (vilt_module.py:270-273): copy q -> k."""
        e = self.engine
        e.k32.copy_(e.q32[: e.layout.ema_end])
        e.lp_stale = True

    def _after_load(self):
        self.engine.lp_stale = True
        if hasattr(self, "proj_queue_ptr"):
            self._queue_ptr_host = None

    # ---- resumable state ---------------------------------------------------------------------
    def training_state(self):
        """Everything OUTSIDE state_dict() that the next step depends on (tensors, numbers, lists and dicts only): the dropout seed
        position (Engine.pass_counter / seed_base), the host copy of the queue pointer, the metric accumulators epoch_wrapup would read,
        and the RNG states - torch CPU and device, and Python's `random` (the RandAugment plan and the collators draw from it).  The
        queue, its pointer, the momentum copies and the Barlow-Twins running statistics are buffers / parameters: state_dict() has them."""
        import random
        e = self.engine
        version, internal, gauss = random.getstate()
        logged = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in self.logged.items()
                  if torch.is_tensor(v) or isinstance(v, (int, float))}
        st = {"pass_counter": int(e.pass_counter), "seed_base": int(e.seed_base),
              "queue_ptr": int(self.queue_ptr) if hasattr(self, "proj_queue_ptr") else None,
              "logged": logged,
              "mlm_epoch_counts": {k: v.detach().cpu() for k, v in getattr(self, "mlm_epoch_counts", {}).items()},
              "mpp_epoch_counts": {k: v.detach().cpu() for k, v in getattr(self, "mpp_epoch_counts", {}).items()},
              "torch_rng": torch.get_rng_state(),
              "python_rng": [int(version), [int(x) for x in internal], gauss]}
        if e.q32.is_cuda:
            st["device_rng"] = torch.cuda.get_rng_state(e.q32.device)
        if self.epoch_metrics is not None:
            st["epoch_metrics"] = self.epoch_metrics.state_dict()
        return st

    def load_training_state(self, state):
        import random
        e = self.engine
        e.pass_counter, e.seed_base = int(state["pass_counter"]), int(state["seed_base"])
        if hasattr(self, "proj_queue_ptr") and state.get("queue_ptr") is not None:
            self._queue_ptr_host = int(state["queue_ptr"])        # (the device copy is a buffer of state_dict())
        self.logged = {k: (v.to(e.device) if torch.is_tensor(v) else v) for k, v in state.get("logged", {}).items()}
        for name in ("mlm_epoch_counts", "mpp_epoch_counts"):
            if state.get(name):
                setattr(self, name, {k: v.to(e.device) for k, v in state[name].items()})
        if self.epoch_metrics is not None:
            self.epoch_metrics.load_state_dict(state.get("epoch_metrics"))      # (a state without the key: an empty table)
        torch.set_rng_state(state["torch_rng"].cpu().to(torch.uint8))
        if "device_rng" in state and e.q32.is_cuda:
            torch.cuda.set_rng_state(state["device_rng"].cpu().to(torch.uint8), e.q32.device)
        version, internal, gauss = state["python_rng"]
        random.setstate((int(version), tuple(int(x) for x in internal), gauss))

    # ---- Lightning shims -------------------------------------------------------------------
    @property
    def device(self):
        return self.engine.device

    def log(self, name, value):
        self.logged[name] = value

    @property
    def queue_ptr(self) -> int:
        if self._queue_ptr_host is None:
            self._queue_ptr_host = int(self.proj_queue_ptr)
        return self._queue_ptr_host

    @queue_ptr.setter
    def queue_ptr(self, v: int):
        self._queue_ptr_host = int(v)
        self.proj_queue_ptr.fill_(int(v))

    def after_backward(self, overlap: bool = False):
        """DDP replacement (run.py:96).  Called by every deferred-backward closure right after its HIP backward has been
        ENQUEUED.  The arena is reduced once per step, after the LAST closure (dist_utils.StepGradSync): with a single
        closure (the MoCo image-view step) as per-layer all-reduces gated on the backward's gradient-ready events
        (overlap=True), otherwise as one blocking pass over the arena."""
        e = self.engine
        factory = None
        if overlap and e.g32.is_cuda and os.environ.get("RMCL_NO_GRAD_OVERLAP", "0") != "1":
            lay = e.layout

            def gate(layer, stream):
                check(lib.rmcl_grad_ready_wait(int(layer), C.c_void_p(stream.cuda_stream)), "grad_ready_wait")

            def factory():
                buckets = dist_utils.grad_buckets(int(lay.layer0), int(lay.layer_stride), int(self.hparams.config["num_layers"]),
                                                  int(e.g32.numel()))
                return dist_utils.GradSync(e.g32, buckets, e.comm_stream, gate, prescaled=True,
                                           compress=self.hparams.config.get("grad_allreduce_dtype"),
                                           algo=self.hparams.config.get("grad_allreduce_algo", "ring"))

        self.step_sync.closure_done(e.g32, enabled=self.sync_grads, overlap=factory)

    def grad_prescale(self) -> float:
        """Registers one deferred backward with the step's gradient reducer and returns 1 / world_size: the mean over
        ranks is applied to the loss gradient of EVERY closure (objectives._DeferredBackward), also on micro-steps
        whose reduction is skipped (sync_grads=False: gradient accumulation)."""
        return self.step_sync.register()

    def wait_grad_sync(self):
        """Make the current stream wait for the overlapped gradient all-reduces (the optimizer calls this)."""
        self.step_sync.wait()

    def zero_grad(self, set_to_none: bool = False):
        self.engine.zero_grads()

    # ---- inference API ---------------------------------------------------------------------
    def _infer(self, batch, key, mask_text, mask_image, image_token_type_idx, image_embeds, image_masks):
        if mask_image:
            if self.engine.mpp is None:
                raise NotImplementedError("MPP masking (mask_image=True) needs a model built with loss_names['mpp'] > 0")
            if key or mask_text or image_embeds is not None or image_masks is not None or image_token_type_idx != 1:
                raise NotImplementedError("infer(mask_image=True) is built for the query pass on pixels alone (not infer_k, mask_text, "
                                          "image_embeds or another token type)")
            return self._infer_mpp(batch)
        if image_embeds is not None or image_masks is not None:
            if mask_text:
                raise NotImplementedError("infer(mask_text=True, image_embeds=...) is not built (the reference never calls it)")
            return self._infer_embeds(batch, key, image_token_type_idx, image_embeds, image_masks)
        if image_token_type_idx not in (1, 2):
            raise NotImplementedError(f"image_token_type_idx={image_token_type_idx}: only 1 and 2 (NLVR2) exist")
        eng = self.engine
        if image_token_type_idx == 2 and eng.nlvr2 is None:
            # the reference's 2-row Embedding raises an IndexError for row 2: only NLVR2 models have the third row
            raise ValueError("image_token_type_idx=2 needs an NLVR2 model (loss_names nlvr2 / nlvr2_attacked: 3-row token_type_embeddings)")
        imgkey = f"image_{image_token_type_idx - 1}" if f"image_{image_token_type_idx - 1}" in batch else "image"   # vilt_module.py:284-287
        eng.dropout_on = self.training and eng.drop_p > 0
        do_mlm = "_mlm" if mask_text else ""                     # vilt_module.py:289-291: the masked ids and their labels
        text_ids, text_masks = batch[f"text_ids{do_mlm}"], batch["text_masks"]
        # the reference's infer is an ordinary differentiable forward (vilt_module.py:275-351): with autograd on, the query pass keeps
        # the FULL stash and the returned features carry a backward into the gradient arena (the momentum pass never does: k_* get no
        # gradients, vilt_module.py:270-273)
        need_grad = (not key) and torch.is_grad_enabled()
        # every differentiable call whose backward is still pending keeps its OWN FULL stash (a second infer() of the same batch
        # size must not overwrite the activations the first one's backward will read); the slot is returned by the backward, or
        # when autograd drops the graph
        slot = self._infer_slot_take() if need_grad else None
        pb = eng.bind_batch(text_ids, text_masks, batch[imgkey][0], tag=f"infer{slot}" if need_grad else "moco")
        pb.d.img_type = image_token_type_idx
        op = eng.make_operand(pb)
        eng.encoder_forward(pb, key=key, mode=L.MODE_FULL if need_grad else L.MODE_INFER, patchesT=op)
        eng.heads_forward(pb, key=key, want_q=False)
        d = pb.d
        N = d.L + 1 + d.P
        x = pb.xn.view(pb.B, N, d.D)
        if pb.geom is None:
            g = self.config["image_size"] // self.config["patch_size"]
            ii, jj = torch.meshgrid(torch.arange(g), torch.arange(g), indexing="ij")
            patch_index = torch.stack([ii, jj], dim=-1).reshape(1, g * g, 2).expand(pb.B, -1, -1)
            grid_hw = (g, g)
        else:                                                  # zero-padded batch: (row, col) of every selected slot
            sel = pb.geom.sel[:, : pb.geom.n].to(torch.int64)
            patch_index = torch.stack([sel // pb.geom.gw, sel % pb.geom.gw], dim=-1)
            grid_hw = (pb.geom.gh, pb.geom.gw)
        feats = (x[:, : d.L].clone(), x[:, d.L:].clone(), pb.cls.clone(), x[:, 0].clone())
        if need_grad:
            def backward(g_txt, g_img, g_cls, g_raw, pb=pb, op=op, N=N):
                dxn = torch.zeros(pb.B, N, d.D, device=eng.device)
                if g_txt is not None:
                    dxn[:, : d.L] += g_txt.to(torch.float32)
                if g_img is not None:
                    dxn[:, d.L:] += g_img.to(torch.float32)
                if g_raw is not None:
                    dxn[:, 0] += g_raw.to(torch.float32)
                dcls = torch.zeros(pb.B, d.D, device=eng.device) if g_cls is None else g_cls.to(torch.float32).contiguous()
                eng.heads_backward(pb, None, dcls, with_grads=True)          # pooler: tanh(W x[:, 0] + b) (heads.py:10-20)
                dxn[:, 0] += pb.dcls
                eng.encoder_backward(pb, L.MODE_FULL, op, dxn.view(pb.B * N, d.D), cls_only=False, dpatches=None)
                self.after_backward()

            # the step belongs to whoever opened it (forward() / training_step); a stand-alone infer() opens one only when no
            # deferred backward of an earlier call is still outstanding - it never wipes their registrations
            if self.step_sync.open <= 0:
                self.step_sync.begin_step()
            feats = _InferFeatures.apply(self.grad_anchor, _SlotClosure(backward, self._infer_busy, slot), self.grad_prescale(), *feats)
        ret = {
            "text_feats": feats[0],
            "image_feats": feats[1],
            "cls_feats": feats[2],
            "raw_cls_feats": feats[3],
            "image_masks": pb.co_mask[:, d.L:].to(torch.int64),
            "text_ids": text_ids,
            "text_masks": text_masks,
            "patch_index": (patch_index, grid_hw),
        }
        if not key:
            ret["image_labels"] = None
            ret["text_labels"] = batch.get(f"text_labels{do_mlm}")
        return ret

    def _infer_mpp(self, batch):
        """infer(batch, mask_image=True) (vilt_module.py:296-306 with mask_it): the pass compute_mpp runs, as an inference call - the features
        carry no backward (train through compute_mpp / training_step).  image_labels [B, 1 + P, 3] as the reference builds them."""
        eng = self.engine
        eng.dropout_on = self.training and eng.drop_p > 0
        pb, mp, _, _ = objectives._mpp_pass(self, batch, batch["text_ids"], "mpp_infer", L.MODE_INFER)
        eng.heads_forward(pb, key=False, want_q=False)
        d = pb.d
        x = pb.xn.view(pb.B, d.L + 1 + d.P, d.D)
        return {
            "text_feats": x[:, : d.L].clone(), "image_feats": x[:, d.L:].clone(), "cls_feats": pb.cls.clone(), "raw_cls_feats": x[:, 0].clone(),
            "image_labels": objectives.mpp_image_labels(mp), "image_masks": pb.co_mask[:, d.L:].to(torch.int64),
            "text_labels": batch.get("text_labels"), "text_ids": batch["text_ids"], "text_masks": batch["text_masks"], "patch_index": None,
        }

    def _infer_embeds(self, batch, key, image_token_type_idx, image_embeds, image_masks):
        """infer(batch, image_embeds=..., image_masks=...) (vilt_module.py:296-313): the image tokens are a visual_embed output instead
        of pixels.  Inference only, like every use the reference makes of it (compute_irtr_recall, under no_grad)."""
        if key:
            raise NotImplementedError("infer_k(image_embeds=...) is not built (the reference never calls it)")
        if torch.is_grad_enabled():
            raise ValueError("infer(image_embeds=..., image_masks=...) runs only under torch.no_grad(): the cached rank pass keeps no "
                             "activations for a backward (the reference uses this shortcut in compute_irtr_recall only, under no_grad)")
        if image_embeds is None or image_masks is None:
            raise ValueError("infer: image_embeds and image_masks must be given together")
        if image_token_type_idx != 1:
            raise NotImplementedError("infer(image_embeds=...): only image_token_type_idx=1")
        eng = self.engine
        eng.dropout_on = False
        text_ids, text_masks = batch["text_ids"], batch["text_masks"]
        B = int(text_ids.shape[0])
        if image_embeds.dim() != 3 or image_embeds.shape[0] != B or tuple(image_masks.shape) != tuple(image_embeds.shape[:2]):
            raise ValueError(f"infer: image_embeds [B, 1 + n, D] / image_masks [B, 1 + n] expected for {B} texts (got {tuple(image_embeds.shape)}, "
                             f"{tuple(image_masks.shape)})")
        if B > 1 and image_embeds.stride(0) == 0 and image_masks.stride(0) == 0:
            # one image expanded over the batch (compute_irtr_recall's `_ie.expand(fblen, l, c)`): one cache slot, every sequence names it
            emb, msk = image_embeds[:1], image_masks[:1]
            img_of = torch.zeros(B, dtype=torch.int32, device=eng.device)
        else:
            emb, msk = image_embeds, image_masks
            img_of = torch.arange(B, dtype=torch.int32, device=eng.device)
        emb = emb.to(eng.device, torch.float32).contiguous()
        msk = msk.to(eng.device, torch.int32).contiguous()
        n = int(emb.shape[1]) - 1
        rp = eng.rank_forward(text_ids, text_masks, emb, msk, img_of, n, cls_tail=False)
        d = rp.d
        x = rp.xn.view(B, d.L + 1 + d.P, d.D)
        return {
            "text_feats": x[:, : d.L].clone(), "image_feats": x[:, d.L:].clone(), "cls_feats": rp.cls.clone(), "raw_cls_feats": x[:, 0].clone(),
            "image_labels": None, "image_masks": rp.co_mask[:, d.L:].to(torch.int64), "text_labels": batch.get("text_labels"),
            "text_ids": text_ids, "text_masks": text_masks, "patch_index": None,
        }

    @torch.no_grad()
    def visual_embed(self, images, max_image_len=None, mask_it=False, select=None, mpp_masks=None):
        """VisionTransformer.visual_embed (vision_transformer.py:559-677) as the reference's compute_irtr_recall calls it: patch embedding
        + resized position rows + cls token, WITHOUT the token-type row.  Returns (image_embeds [B, 1 + n, D] fp32, image_masks [B, 1 + n],
        (patch_index, (H, W)), None).  max_image_len None: the config's.  select: the caller's patch draw (parity tests)."""
        if mask_it and self.engine.mpp is None:
            raise NotImplementedError("visual_embed(mask_it=True) (MPP masking) needs a model built with loss_names['mpp'] > 0")
        ps = self.config["patch_size"]
        if mask_it:
            return self._visual_embed_mpp(images, max_image_len, select, mpp_masks)
        emb, msk, patch_index = self.engine.visual_embed(images, max_image_len=max_image_len, select=select)
        return emb, msk, (patch_index, (int(images.shape[2]) // ps, int(images.shape[3]) // ps)), None

    def _visual_embed_mpp(self, images, max_image_len, select, mpp_masks=None):
        """visual_embed(mask_it=True): the reference's order - the two mask draws (or the caller's `mpp_masks` = (masked, replaced) [B, G]),
        then the patch selection -, the embeddings with the mask token in place of the replaced patches, and the label [B, 1 + n, 3] as the
        fourth value.  Labels and masks take the path of compute_mpp (Engine.mpp_bind)."""
        from ...runtime import mpp_draw_masks
        eng, ps = self.engine, self.config["patch_size"]
        img = images.to(eng.device, torch.float32).contiguous() if torch.is_tensor(images) else eng.u8_on_device(images)   # (byte feeds stay bytes)
        B, _, Hh, Ww = img.shape
        masks = mpp_masks if mpp_masks is not None else mpp_draw_masks(B, (Hh // ps) * (Ww // ps))
        emb, msk, patch_index, mp = eng.visual_embed(img, max_image_len=max_image_len, select=select, mpp_masks=masks)
        return emb, msk, (patch_index, (Hh // ps, Ww // ps)), objectives.mpp_image_labels(mp)

    def _infer_slot_take(self) -> int:
        for slot in range(self.MAX_PENDING_INFER):
            if slot not in self._infer_busy:
                self._infer_busy.add(slot)
                return slot
        raise RuntimeError(f"infer(): {self.MAX_PENDING_INFER} differentiable calls are still waiting for their backward (each keeps a full "
                           "activation stash); back-propagate or drop their outputs first, or call infer() under torch.no_grad() for inference")

    def infer(self, batch, mask_text=False, mask_image=False, image_token_type_idx=1, image_embeds=None, image_masks=None):
        """vilt_module.py:275-351.  Differentiable like the reference's when autograd is on (``text_feats`` / ``image_feats`` /
        ``cls_feats`` / ``raw_cls_feats`` back-propagate into every query parameter's ``.grad``); ``torch.no_grad()`` gives the
        stash-free inference pass.  The ``image_embeds`` shortcut (pre-computed visual_embed output, used by the reference's
        downstream tasks only) runs under ``torch.no_grad()`` only (``_infer_embeds``)."""
        return self._infer(batch, False, mask_text, mask_image, image_token_type_idx, image_embeds, image_masks)

    @torch.no_grad()
    def infer_k(self, batch, mask_text=False, mask_image=False, image_token_type_idx=1, image_embeds=None, image_masks=None):
        return self._infer(batch, True, mask_text, mask_image, image_token_type_idx, image_embeds, image_masks)

    def forward(self, batch):
        self.step_sync.begin_step()
        self.engine.dropout_on = self.training and self.engine.drop_p > 0
        ret = dict()
        if len(self.current_tasks) == 0:
            ret.update(self.infer(batch))
            return ret
        if "mlm" in self.current_tasks:                                   # first, like the reference (vilt_module.py:426-436)
            ret.update(objectives.compute_mlm(self, batch))
        if "mpp" in self.current_tasks:                                   # second, like the reference (vilt_module.py:430-432)
            ret.update(objectives.compute_mpp(self, batch))
        if "itm" in self.current_tasks:
            ret.update(objectives.compute_itm_wpa(self, batch))
        if "moco" in self.current_tasks:
            ret.update(objectives.compute_moco_contrastive(self, batch))
        if "barlowtwins" in self.current_tasks:
            ret.update(objectives.compute_barlowtwins_contrastive(self, batch))
        if "vqa" in self.current_tasks:
            ret.update(objectives.compute_vqa(self, batch))
        if "vqa_attacked" in self.current_tasks:
            ret.update(objectives.compute_vqa_attack(self, batch))
        if "nlvr2" in self.current_tasks:
            ret.update(objectives.compute_nlvr2(self, batch))
        if "nlvr2_attacked" in self.current_tasks:
            ret.update(objectives.compute_nlvr2_attack(self, batch))
        if "irtr" in self.current_tasks:
            ret.update(objectives.compute_irtr(self, batch))
        unsupported = [t for t in self.current_tasks if t not in ("mlm", "mpp", "itm", "moco", "barlowtwins", "vqa", "vqa_attacked", "nlvr2", "nlvr2_attacked", "irtr")]
        if unsupported:
            raise NotImplementedError(f"tasks {unsupported} are outside the RMCL hot path (SURVEY 8)")
        return ret

    def training_step(self, batch, batch_idx):
        vilt_utils.set_task(self)
        output = self(batch)
        total_loss = sum([v for k, v in output.items() if "loss" in k])
        return total_loss

    def training_epoch_end(self, outs=None):
        vilt_utils.epoch_wrapup(self)

    def validation_step(self, batch, batch_idx):
        vilt_utils.set_task(self)
        with torch.no_grad():
            return self(batch)

    def validation_epoch_end(self, outs=None):
        vilt_utils.epoch_wrapup(self)

    def test_epoch_end(self, outs=None):
        vilt_utils.epoch_wrapup(self)

    def test_step(self, batch, batch_idx):
        output = self.validation_step(batch, batch_idx)
        if "vqa_preds" in output:                                          # vqa_test_step (objectives.py:1519-1530)
            preds = output["vqa_preds"].tolist()
            if self.id2answer is not None:
                preds = [self.id2answer[i] for i in preds]
            return {"qids": batch["qid"], "preds": preds}
        return output

    def configure_optimizers(self):
        return vilt_utils.set_schedule(self)
