"""CPU oracle of the masked-language-modelling step (test infrastructure): the reference's MLMHead (heads.py:183-195), compute_mlm's
cross-entropy (objectives.py:604-630) and its Accuracy metric (gadgets/my_metrics.py:5-28) restated in torch on top of
oracle.rmcl_oracle (infer / layer_norm / gelu_erf).  Also the seeded head weights and the seeded masking that tools/gen_golden_mlm.py
feeds the reference, so every mlm_* fixture is reproducible from (cfg, seeds) without the reference - decoder.weight (94 MB) is never
stored, only seeded."""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from oracle import rmcl_oracle as O

MASK_ID = 103            # [MASK] of bert-base-uncased
MODES = ("random", "ragged", "empty")
N_SAMPLE_COLS = 256      # logit columns per masked row recorded in a fixture


def mlm_param_shapes(cfg: dict) -> List[Tuple[str, Tuple[int, ...]]]:
    """MLMHead(bert_config) without a tied weight (vilt_module.py:56): six tensors."""
    D, V = cfg["hidden_size"], cfg["vocab_size"]
    return [("mlm_score.bias", (V,)), ("mlm_score.transform.dense.weight", (D, D)), ("mlm_score.transform.dense.bias", (D,)),
            ("mlm_score.transform.LayerNorm.weight", (D,)), ("mlm_score.transform.LayerNorm.bias", (D,)),
            ("mlm_score.decoder.weight", (V, D))]


def dominant_tokens(cfg: dict, seed: int) -> Tuple[int, int]:
    """The two vocabulary ids whose output bias mlm_init_params raises (6 and 2).  Random 0.02-scale logits over 30522 classes have
    a top-two gap of about sigma / sqrt(2 ln V) - far below the bf16 logits tolerance on most rows - so a fixture with a DECIDED
    argmax needs structure: with these two bumps every row's first and second maximum are 4 +- 0.8 apart."""
    g = torch.Generator().manual_seed(seed + 7919)
    t = torch.randperm(cfg["vocab_size"] - 1000, generator=g)[:2] + 1000
    return int(t[0]), int(t[1])


def mlm_init_params(cfg: dict, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded head weights: the reference's init_weights distribution for the matrices (N(0, 0.02)), with non-trivial biases and
    LayerNorm affine terms so that their gradients are exercised off the init point, and the two raised output biases of
    ``dominant_tokens``."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in mlm_param_shapes(cfg):
        if name.endswith("LayerNorm.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t.float()
    t1, t2 = dominant_tokens(cfg, seed)
    out["mlm_score.bias"][t1] = 6.0
    out["mlm_score.bias"][t2] = 2.0
    return out


def synthetic_mlm(batch: dict, seed: int, vocab: int, mode: str = "random", dup_label: int = None, mlm_prob: float = 0.15) -> dict:
    """text_ids_mlm / text_labels_mlm for an O.synthetic_batch, by the BERT rule (chosen with probability mlm_prob among the valid
    positions; 80 % [MASK], 10 % random id, 10 % unchanged).  mode "ragged" (B >= 4) pins the edge cases: sample 0 has NO masked token,
    sample 1 masks its first token, sample 2 its last valid token, and positions (1, 3) and (3, 2) carry the same original id
    `dup_label` (one label in two rows).  mode "empty": nothing is masked (n = 0).  Returns a new batch dict."""
    assert mode in MODES, mode
    g = torch.Generator().manual_seed(seed)
    ids = batch["text_ids"].clone()
    masks = batch["text_masks"]
    B, L = ids.shape
    chosen = (torch.rand(B, L, generator=g) < mlm_prob) & masks.bool()
    kind = torch.rand(B, L, generator=g)
    rnd = torch.randint(0, vocab, (B, L), generator=g, dtype=torch.int64)
    if mode == "empty":
        chosen[:] = False
    if mode == "ragged":
        assert B >= 4
        lens = masks.sum(dim=1)
        chosen[0] = False
        chosen[1, 0] = True
        chosen[2, int(lens[2]) - 1] = True
        dup = int(ids[1, 3]) if dup_label is None else int(dup_label)
        ids[1, 3] = dup
        ids[3, 2] = dup
        chosen[1, 3] = True
        chosen[3, 2] = True
    labels = torch.where(chosen, ids, torch.full_like(ids, -100))
    out = ids.clone()
    out[chosen & (kind < 0.8)] = MASK_ID
    swap = chosen & (kind >= 0.8) & (kind < 0.9)
    out[swap] = rnd[swap]
    nb = dict(batch)
    nb["text_ids"] = ids
    nb["text_ids_mlm"] = out
    nb["text_labels_mlm"] = labels
    return nb


def compact(labels: torch.Tensor, N: int):
    """The compaction restated in numpy: (row b * N + l of every labelled position in ascending order, their labels, n)."""
    import numpy as np
    lab = labels.numpy()
    B, L = lab.shape
    pos = np.flatnonzero(lab.reshape(-1) != -100)
    return (pos // L) * N + pos % L, lab.reshape(-1)[pos], int(pos.size)


def mlm_transform(p: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """BertPredictionHeadTransform: Linear - exact-erf GELU - LayerNorm(eps 1e-12)."""
    a = x @ p["mlm_score.transform.dense.weight"].t() + p["mlm_score.transform.dense.bias"]
    return O.layer_norm(O.gelu_erf(a), p["mlm_score.transform.LayerNorm.weight"], p["mlm_score.transform.LayerNorm.bias"], 1e-12)


def mlm_head(p: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """MLMHead.forward (heads.py:191-195): decoder(transform(x)) + bias."""
    return mlm_transform(p, x) @ p["mlm_score.decoder.weight"].t() + p["mlm_score.bias"]


def mlm_loss(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    return F.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100)


def mlm_accuracy(logits: torch.Tensor, labels: torch.Tensor) -> Tuple[int, int]:
    """Accuracy.update (my_metrics.py:12-24): (correct, total) over the positions whose label is not -100."""
    on = labels != -100
    pred = logits.detach().argmax(dim=-1)
    return int((pred[on] == labels[on]).sum()), int(on.sum())


def compute_mlm(p, cfg, batch, dense: bool = False) -> dict:
    """compute_mlm (objectives.py:604-630).  The logits are formed on the labelled rows only unless `dense` (cross_entropy ignores
    the others, so loss and gradients are the reference's): a [64, 40, 30522] fp32 tensor and its autograd copies are 1 GB on the CPU."""
    out = O.infer(p, cfg, batch["text_ids_mlm"], batch["text_masks"], batch["image"][0])
    labels = batch["text_labels_mlm"]
    feats = out["text_feats"]
    on = labels != -100
    rows = mlm_head(p, feats[on])                                      # [n, V], ascending (b, l)
    loss = F.cross_entropy(rows, labels[on], reduction="sum") / on.sum()          # n = 0: 0 / 0 = NaN like ignore_index on an empty set
    correct = int((rows.detach().argmax(dim=-1) == labels[on]).sum())
    ret = {"mlm_loss": loss, "mlm_rows": rows, "mlm_labels": labels, "mlm_ids": batch["text_ids_mlm"], "text_feats": feats,
           "correct": correct, "n": int(on.sum()), "row_loss": F.cross_entropy(rows, labels[on], reduction="none")}
    if dense:
        ret["mlm_logits"] = mlm_head(p, feats)
    return ret


FIXTURES = ("mlm_L12_B2", "mlm_L2_B4_ragged", "mlm_itm_L2_B4", "mlm_L2_B2_empty")


def sample_columns(cfg: dict, seed: int, labels: torch.Tensor) -> torch.Tensor:
    """The recorded logit columns of a fixture: the two dominant tokens, every label of the batch, then seeded random ids."""
    g = torch.Generator().manual_seed(seed + 104729)
    t1, t2 = dominant_tokens(cfg, seed)
    lab = labels[labels != -100].unique().tolist()
    rest = torch.randint(0, cfg["vocab_size"], (N_SAMPLE_COLS,), generator=g).tolist()
    cols = list(dict.fromkeys([t1, t2] + lab + rest))[:N_SAMPLE_COLS]
    return torch.tensor(cols, dtype=torch.int64)


def load_case(name: str):
    """An mlm_* fixture with everything needed to recompute it: (fixture, cfg, params incl. the head, batch with text_ids_mlm /
    text_labels_mlm, with_itm?)."""
    from tests.golden_util import load
    g = load(name + ".npz")
    B, sw, sh, sb, sm, ragged, L, mode, with_itm = [int(x) for x in g["meta"]]
    cfg = O.default_config(num_layers=L, num_negative=1024 if L == 2 else 65536, per_gpu_batchsize=B)
    p = dict(O.init_params(cfg, sw), **mlm_init_params(cfg, sh))
    batch = O.synthetic_batch(cfg, B, sb, ragged_text=bool(ragged))
    batch = synthetic_mlm(batch, sm, cfg["vocab_size"], MODES[mode], dup_label=dominant_tokens(cfg, sh)[0])
    return g, cfg, p, batch, bool(with_itm)
