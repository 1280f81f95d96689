"""Generate the NLVR2 golden fixtures tests/golden/nlvr2_*.npz by running the REFERENCE's own compute_nlvr2 / compute_nlvr2_attack /
PGDAttack_nlvr2 (vilt/modules/objectives.py:898-1060, attack/pgd_attack_vilt.py:241-342) and its nn.Sequential head (vilt_module.py:193-200)
with a 3-row token_type_embeddings (:201-205).

TEST INFRASTRUCTURE ONLY: runs on the build machine only (needs the reference checkout that oracle/gen_golden.py imports).  It imports
oracle.gen_golden (its stand-ins, Holder, tensor_digest) and oracle.rmcl_oracle unchanged; the head weights, the perturbed third
token-type row and the pair batches come from tests/nlvr2_oracle.py (seeded), so every fixture is reproducible without the reference.

The reference's train branch of compute_nlvr2_attack reads ret["nlvr2_attacked_labels"], which it never sets (objectives.py:944-946): the
attacked fixtures therefore run in the val phase, with table_name mixing dev and test rows.  drop_rate is 0, so the arithmetic is the
train phase's; the gradients are those of nlvr2_original_loss + nlvr2_attacked_loss (what training_step would sum).

Also the reference's NLVR2Dataset (vilt/datasets/nlvr2_dataset.py) on two tiny arrow shards written here (tests/golden/nlvr2_dev.arrow,
nlvr2_test1.arrow) -> tests/golden/nlvr2_dataset.npz.

Usage:  python tools/gen_golden_nlvr2.py [fixture names | dataset]      (writes tests/golden/nlvr2_*, ~1 min)
"""
from __future__ import annotations

import os
import sys
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins, imports the reference)
from attack.pgd_attack_vilt import PGDAttack_nlvr2  # noqa: E402  (reference, unmodified)
from tests import golden_util  # noqa: E402
from tests import nlvr2_oracle as N  # noqa: E402


def _holder(cfg, p, idx):
    h = G.Holder(cfg)
    D = cfg["hidden_size"]
    h.nlvr2_classifier = nn.Sequential(nn.Linear(2 * D, 2 * D), nn.LayerNorm(2 * D), nn.GELU(), nn.Linear(2 * D, 2))
    h.token_type_embeddings = nn.Embedding(3, D)
    h.image_view, h.text_view = True, False
    h.attack_idx = list(idx) if idx else [True, True]
    h.pgd_attacker = PGDAttack_nlvr2(dict(cfg, attack_idx=h.attack_idx))
    acc = lambda lg, lb: (lg.argmax(-1) == lb).float().mean()
    chg = lambda la, lo: (la.argmax(-1) != lo.argmax(-1)).float().mean()
    for ph in ("train", "dev", "test"):
        for t in ("nlvr2", "nlvr2_original", "nlvr2_attacked"):
            setattr(h, f"{ph}_{t}_loss", lambda x: x)
            setattr(h, f"{ph}_{t}_accuracy", acc)
        setattr(h, f"{ph}_nlvr2_attacked_change_rate_cross", chg)
    h.load_oracle_params({n: t for n, t in p.items() if not n.startswith(("k_", "moco_head", "itm_score"))})
    return h


def run(name):
    torch.manual_seed(888)
    cfg, p, batch, idx = N.case_inputs(name)
    cfg = dict(cfg, image_view=True, text_view=False)
    h = _holder(cfg, p, idx)
    attacked = idx is not None
    params = [(n, prm) for n, prm in h.named_parameters() if not n.startswith("k_")]
    deltas = []
    attack = h.pgd_attacker.pgd_attack

    def recording_attack(pl_module, b_, **kw):
        d = attack(pl_module, b_, **kw)
        deltas.append(tuple(x.detach().clone() for x in d))
        return d

    h.pgd_attacker.pgd_attack = recording_attack
    h.zero_grad()
    if attacked:
        h.eval()                                               # val phase (defect (a) of the train branch)
        ret = G.objectives.compute_nlvr2_attack(h, deepcopy(batch))
        total = ret["nlvr2_original_loss"] + ret["nlvr2_attacked_loss"]
    else:
        h.train()
        ret = G.objectives.compute_nlvr2(h, deepcopy(batch))
        total = ret["nlvr2_loss"]
    total.backward()
    out = {"answers": np.array(batch["answers"], dtype=np.int64), "total_loss": np.float64(total.item())}
    for k, v in ret.items():
        if k.endswith("_loss"):
            out[k] = np.float64(v.item())
        elif k.endswith("_logits"):
            out[k] = v.detach().numpy()
    for kk, v in h.logged.items():
        out["log_" + kk.replace("/", "__")] = np.float64(v)
    gnames, gd = [], []
    for n, prm in params:
        if prm.grad is not None:
            gnames.append(n)
            gd.append(G.tensor_digest(prm.grad))
    out["grad_names"] = np.array(gnames)
    out["grad_digest"] = np.stack(gd)
    if attacked:
        assert len(deltas) == 1
        for k, d in enumerate(deltas[0]):
            out[f"delta{k}_sub"] = d[:, :, ::8, ::8].contiguous().numpy()
            out[f"delta{k}_digest"] = G.tensor_digest(d)
    hc = h.nlvr2_classifier
    out["grad_nlvr2_w0"] = hc[0].weight.grad[:8, :64].numpy().copy()
    out["grad_nlvr2_b0"] = hc[0].bias.grad[:64].numpy().copy()
    out["grad_nlvr2_g1"] = hc[1].weight.grad[:64].numpy().copy()
    out["grad_nlvr2_w3"] = hc[3].weight.grad[:, :64].numpy().copy()
    out["grad_nlvr2_b3"] = hc[3].bias.grad.numpy().copy()
    out["grad_token_type"] = h.token_type_embeddings.weight.grad.numpy().copy()
    out["grad_pooler_w"] = h.pooler.dense.weight.grad[:8, :64].numpy().copy()
    out["grad_qkv0_w"] = h.transformer.blocks[0].attn.qkv.weight.grad[:8, :64].numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
    golden_util.save(path, out)
    print(os.path.basename(path), {k: float(v) for k, v in out.items() if k.endswith("_loss")},
          {k: float(v) for k, v in out.items() if k.startswith("log_")})


def write_nlvr2_shard(path, rows):
    """rows: (png image_0, png image_1, [statements], ["True" / "False" per statement]) - the columns of the reference's
    write_nlvr2 (vilt/utils/write_nlvr2.py: image_0, image_1, questions, answers, identifier)"""
    import pyarrow as pa
    t = pa.table({"image_0": pa.array([r[0] for r in rows], type=pa.binary()), "image_1": pa.array([r[1] for r in rows], type=pa.binary()),
                  "questions": pa.array([r[2] for r in rows], type=pa.list_(pa.string())),
                  "answers": pa.array([r[3] for r in rows], type=pa.list_(pa.string())),
                  "identifier": pa.array([f"pair-{i}" for i in range(len(rows))])})
    with pa.OSFile(path, "wb") as sink:
        with pa.RecordBatchFileWriter(sink, t.schema) as writer:
            writer.write_table(t)


def toy_png(w, h, seed):
    import io
    from PIL import Image
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = (120 + 70 * np.sin(xx / 7.0)[..., None] * np.cos(yy / 5.0)[..., None] + rng.normal(0, 15, (h, w, 3))).clip(0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG")
    return buf.getvalue()


def run_dataset():
    import importlib.util
    import types
    import pyarrow as pa
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.attack import word_substitution as WS
    gold = os.path.join(ROOT, "tests", "golden")
    write_nlvr2_shard(os.path.join(gold, "nlvr2_dev.arrow"), [
        (toy_png(64, 48, 1), toy_png(40, 72, 2), ["two dog near the house", "the man by a car"], ["True", "False"]),
        (toy_png(56, 56, 3), toy_png(80, 40, 4), ["a child in the home"], ["False"])])
    write_nlvr2_shard(os.path.join(gold, "nlvr2_test1.arrow"), [
        (toy_png(48, 64, 5), toy_png(64, 64, 6), ["some woman at the road", "three kid from the cottage", "his puppy over the lane"],
         ["True", "True", "False"])])
    spec = importlib.util.spec_from_file_location("ref_transforms_utils3", os.path.join(G.REF, "vilt", "transforms", "utils.py"))
    tu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tu)

    def ref_transform(size):
        r = tu.MinMaxResize(shorter=size, longer=int((1333 / 800) * size))
        def f(img):
            t = torch.from_numpy(np.asarray(r(img)).copy()).permute(2, 0, 1).float().div(255.0)
            return (t - 0.5) / 0.5
        return f
    sys.modules["vilt.transforms"] = types.ModuleType("vilt.transforms")
    sys.modules["vilt.transforms"].keys_to_transforms = lambda keys, size=224: [ref_transform(size) for _ in keys]
    pkg = types.ModuleType("ref_nlvr2pkg")
    pkg.__path__ = [os.path.join(G.REF, "vilt", "datasets")]
    sys.modules["ref_nlvr2pkg"] = pkg
    spec = importlib.util.spec_from_file_location("ref_nlvr2pkg.base_dataset", os.path.join(G.REF, "vilt", "datasets", "base_dataset.py"))
    bd = importlib.util.module_from_spec(spec)
    sys.modules["ref_nlvr2pkg.base_dataset"] = bd
    spec.loader.exec_module(bd)
    spec = importlib.util.spec_from_file_location("ref_nlvr2pkg.nlvr2_dataset", os.path.join(G.REF, "vilt", "datasets", "nlvr2_dataset.py"))
    nd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nd)
    _concat = pa.concat_tables
    pa.concat_tables = lambda tables, promote=False, **k: _concat(tables, promote_options="default" if promote else "none", **k)
    ds = nd.NLVR2Dataset(gold, ["pixelbert"], 64, split="val")
    ds.tokenizer = WS.load_tokenizer(os.path.join(gold, "toy_vocab.txt"))
    out = {"len": np.array(len(ds)),
           "index_mapper": np.array([[ds.index_mapper[j][0], ds.index_mapper[j][1]] for j in range(len(ds))])}
    for j in range(len(ds)):
        r = ds[j]
        out[f"s{j}_text"] = np.array(r["text"][0])
        out[f"s{j}_ids"] = np.array(r["text"][1]["input_ids"])
        out[f"s{j}_answers"] = np.array(int(r["answers"]))
        out[f"s{j}_table_name"] = np.array(r["table_name"])
        for k in ("image_0", "image_1"):
            out[f"s{j}_{k}_shape"] = np.array(r[k][0].shape)
            out[f"s{j}_{k}_digest"] = G.tensor_digest(r[k][0])
    pa.concat_tables = _concat
    path = os.path.join(gold, "nlvr2_dataset.npz")
    np.savez_compressed(path, **out)
    print("nlvr2 dataset fixture", os.path.getsize(path), "bytes; len", len(ds), [str(out[f"s{j}_table_name"]) for j in range(len(ds))])


if __name__ == "__main__":
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or N.FIXTURES + ("dataset",)):
        if name == "dataset":
            run_dataset()
        else:
            run(name)
