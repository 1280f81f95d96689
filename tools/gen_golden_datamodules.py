"""tests/golden/datamodules.json: what the REFERENCE's own ``VQAv2Dataset`` and ``CocoCaptionKarpathyDataset`` (vilt/datasets/) give on
the toy shards of tests/datamodule_toy.py - shard names, lengths, first / last index entries and the non-image values of a few samples,
false-text draws included, under a seeded ``random``.  Recorded results only; tests/test_datamodules_cpu.py compares the package's
classes against them.

    python tools/gen_golden_datamodules.py [<reference checkout>]        (default: the checkout oracle/gen_golden.py reads)

The reference's modules are loaded with the stand-ins of the dataset fixture generators (oracle/gen_golden.py run_dataset,
tools/gen_golden_nlvr2.py): its ``vilt.transforms`` (torchvision) is replaced by the reference's MinMaxResize + the ToTensor / Normalize
arithmetic, and ``pyarrow.concat_tables(promote=True)`` is spelled for the installed pyarrow.  The reference de-duplicates captions with
``list(set(texts))``, whose order depends on the hash seed: for COCO the file records order-free facts (the caption SET of a sample's
image row and of the rows its false-text draws land in); VQA keeps duplicates and is recorded verbatim."""
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (installs the stand-ins for the reference's missing imports, torchvision among them)

SEED, FALSE_TEXTS, IMAGE_SIZE = 123, 2, 64


def load_reference(ref):
    import pyarrow as pa
    spec = importlib.util.spec_from_file_location("ref_transforms_utils4", os.path.join(ref, "vilt", "transforms", "utils.py"))
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
    pkg = types.ModuleType("ref_dmpkg")
    pkg.__path__ = [os.path.join(ref, "vilt", "datasets")]
    sys.modules["ref_dmpkg"] = pkg
    mods = {}
    for name in ("base_dataset", "coco_caption_karpathy_dataset", "vqav2_dataset"):
        spec = importlib.util.spec_from_file_location(f"ref_dmpkg.{name}", os.path.join(ref, "vilt", "datasets", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"ref_dmpkg.{name}"] = m
        spec.loader.exec_module(m)
        mods[name] = m
    _concat = pa.concat_tables
    pa.concat_tables = lambda tables, promote=False, **k: _concat(tables, promote_options="default" if promote else "none", **k)
    return mods["coco_caption_karpathy_dataset"].CocoCaptionKarpathyDataset, mods["vqav2_dataset"].VQAv2Dataset


def entry(ds, j):
    return [int(ds.index_mapper[j][0]), -1 if ds.index_mapper[j][1] is None else int(ds.index_mapper[j][1])]


def row_of(ds, text):
    rows = [i for i, caps in enumerate(ds.all_texts) if text in caps]
    return sorted(ds.all_texts[rows[0]])


def main(ref):
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.attack.word_substitution import load_tokenizer
    from tests.datamodule_toy import VOCAB, write_toy_root
    Coco, Vqa = load_reference(ref)
    tok = load_tokenizer(VOCAB)
    out = {"seed": SEED, "draw_false_text": FALSE_TEXTS, "image_size": IMAGE_SIZE}
    with tempfile.TemporaryDirectory() as root:
        write_toy_root(root, only=("coco", "vqav2"))
        for key, cls in (("coco", Coco), ("vqa", Vqa)):
            for split in ("train", "val", "test"):
                ds = cls(root, ["pixelbert"], split=split, image_size=IMAGE_SIZE, max_text_len=40, draw_false_image=0,
                         draw_false_text=FALSE_TEXTS if key == "coco" else 0, image_only=False)
                ds.tokenizer = tok
                rec = {"names": list(ds.names), "len": len(ds), "first": entry(ds, 0), "last": entry(ds, len(ds) - 1), "samples": {}}
                random.seed(SEED)
                for j in sorted({0, 1, len(ds) // 2, len(ds) - 1}):
                    s = ds[j]
                    if key == "coco":
                        one = {"meta": [int(s["img_index"]), int(s["cap_index"]), int(s["raw_index"]), int(s["replica"])],
                               "row_captions": sorted(ds.all_texts[s["img_index"]]),
                               "false_rows": [row_of(ds, s[f"false_text_{r}"][0]) for r in range(FALSE_TEXTS)],
                               "keys": sorted(s.keys())}
                        if "iid" in s:
                            one["iid"] = int(s["iid"])
                    else:
                        one = {"text": s["text"][0], "ids": [int(i) for i in s["text"][1]["input_ids"]], "vqa_answer": list(s["vqa_answer"]),
                               "vqa_labels": [int(i) for i in s["vqa_labels"]], "vqa_scores": [float(x) for x in s["vqa_scores"]],
                               "qid": int(s["qid"]), "keys": sorted(s.keys()), "image_shape": list(s["image"][0].shape)}
                    rec["samples"][str(j)] = one
                out[f"{key}_{split}"] = rec
    path = os.path.join(ROOT, "tests", "golden", "datamodules.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("datamodules fixture", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else G.REF)
