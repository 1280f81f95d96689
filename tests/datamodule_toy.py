"""Toy ``data_root`` for the datamodule tests and their fixture generator (tools/gen_golden_datamodules.py): every shard name the
datasets of rmcl_amd.vilt.datasets read, a few rows each, written in the layouts of the reference's write_*.py scripts.  Images are small
PNGs (lossless: the decoded pixels do not depend on the codec version); captions use the words of tests/golden/toy_vocab.txt, with
multi-piece words ("dogs" -> dog ##s)."""
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "toy_vocab.txt")

SUBJECTS = ["two dogs", "the man", "a child", "some woman", "three kids", "his puppy", "a cat", "the lady", "a big dog", "the little kitten"]
VERBS = ["walking near", "played in", "jumped over", "looks at", "sitting by", "running from", "standing on", "holding"]
PLACES = ["the houses", "a car", "the home", "the road", "a green field", "the red boat", "a table", "the street"]


def caption(k: int) -> str:
    return f"{SUBJECTS[k % len(SUBJECTS)]} {VERBS[(k // 3) % len(VERBS)]} {PLACES[(k // 7) % len(PLACES)]}"


def toy_png(w: int, h: int, seed: int) -> bytes:
    from PIL import Image
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = (120 + 70 * np.sin(xx / 7.0)[..., None] * np.cos(yy / 5.0)[..., None] + rng.normal(0, 15, (h, w, 3))).clip(0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG")
    return buf.getvalue()


SIZES = [(80, 60), (60, 80), (64, 64), (90, 50), (48, 72)]                # (w, h) of the toy images, cycled


def _write(path, table):
    import pyarrow as pa
    with pa.OSFile(path, "wb") as sink:
        with pa.RecordBatchFileWriter(sink, table.schema) as writer:
            writer.write_table(table)


def caption_shard(path, n_images, seed, per_image=2, id_prefix="COCO_val2014_"):
    """columns of write_coco_karpathy.py: image, caption, image_id, split; image 1 repeats a caption (remove_duplicate)"""
    import pyarrow as pa
    images, captions = [], []
    for i in range(n_images):
        w, h = SIZES[(seed + i) % len(SIZES)]
        images.append(toy_png(w, h, 100 * seed + i))
        caps = [caption(11 * seed + 3 * i + j) for j in range(per_image)]
        if i == 1:
            caps.append(caps[0])
        captions.append(caps)
    _write(path, pa.table({"image": pa.array(images, type=pa.binary()), "caption": pa.array(captions, type=pa.list_(pa.string())),
                           "image_id": pa.array([f"{id_prefix}{1000 * seed + i:012d}.jpg" for i in range(n_images)]),
                           "split": pa.array(["x"] * n_images)}))


ANSWERS = ["yes", "no", "two", "red", "dog", "car", "green"]                # label = position in this list


def vqa_shard(path, n_images, seed):
    """columns of write_vqa.py: image, questions, answers, answer_labels, answer_scores, image_id, question_id, split; per image a list of
    questions, per question a list of answers / labels / scores.  A question repeated inside an image is kept (remove_duplicate=False)."""
    import pyarrow as pa
    images, qs, ans, labs, scs, qids = [], [], [], [], [], []
    for i in range(n_images):
        w, h = SIZES[(seed + 2 * i) % len(SIZES)]
        images.append(toy_png(w, h, 200 * seed + i))
        nq = 1 + (i + seed) % 3
        q = ["is " + caption(5 * seed + i + j) for j in range(nq)]
        if nq == 3:
            q[2] = q[0]
        qs.append(q)
        la = [[(seed + i + j) % len(ANSWERS)] + ([(seed + i + j + 3) % len(ANSWERS)] if j % 2 else []) for j in range(nq)]
        labs.append(la)
        ans.append([[ANSWERS[x] for x in l] for l in la])
        scs.append([[1.0] + ([0.3] if len(l) > 1 else []) for l in la])
        qids.append([10000 * seed + 10 * i + j for j in range(nq)])
    _write(path, pa.table({"image": pa.array(images, type=pa.binary()), "questions": pa.array(qs, type=pa.list_(pa.string())),
                           "answers": pa.array(ans, type=pa.list_(pa.list_(pa.string()))),
                           "answer_labels": pa.array(labs, type=pa.list_(pa.list_(pa.int64()))),
                           "answer_scores": pa.array(scs, type=pa.list_(pa.list_(pa.float64()))),
                           "image_id": pa.array([1000 * seed + i for i in range(n_images)]),
                           "question_id": pa.array(qids, type=pa.list_(pa.int64())), "split": pa.array(["x"] * n_images)}))


def nlvr2_shard(path, n_rows, seed):
    """columns of write_nlvr2.py: image_0, image_1, questions, answers ("True" / "False"), identifier"""
    import pyarrow as pa
    rows = []
    for i in range(n_rows):
        (w0, h0), (w1, h1) = SIZES[(seed + i) % len(SIZES)], SIZES[(seed + i + 2) % len(SIZES)]
        nq = 1 + (i + seed) % 2
        rows.append((toy_png(w0, h0, 300 * seed + i), toy_png(w1, h1, 300 * seed + 50 + i), [caption(7 * seed + 2 * i + j) for j in range(nq)],
                     ["True" if (seed + i + j) % 2 else "False" for j in range(nq)]))
    _write(path, pa.table({"image_0": pa.array([r[0] for r in rows], type=pa.binary()), "image_1": pa.array([r[1] for r in rows], type=pa.binary()),
                           "questions": pa.array([r[2] for r in rows], type=pa.list_(pa.string())),
                           "answers": pa.array([r[3] for r in rows], type=pa.list_(pa.string())),
                           "identifier": pa.array([f"pair-{seed}-{i}" for i in range(n_rows)])}))


# shard -> (writer, rows, seed).  The validation splits hold a multiple of four entries (whole batches of the toy configs), the COCO one
# twelve images (recall@10 needs ten).  SBU and GCC have only some of their training tables: a missing table is skipped, like the
# reference does
SHARDS = {
    "coco_caption_karpathy_train": (caption_shard, 4, 1), "coco_caption_karpathy_restval": (caption_shard, 3, 2),
    "coco_caption_karpathy_test": (caption_shard, 12, 3), "coco_caption_karpathy_val": (caption_shard, 2, 4),
    "f30k_caption_karpathy_train": (caption_shard, 4, 5), "f30k_caption_karpathy_val": (caption_shard, 2, 6),
    "f30k_caption_karpathy_test": (caption_shard, 3, 7),
    "vg": (caption_shard, 4, 8), "sbu_0": (caption_shard, 3, 9), "sbu_3": (caption_shard, 2, 10),
    "conceptual_caption_train_0": (caption_shard, 3, 11), "conceptual_caption_train_2": (caption_shard, 2, 12),
    "conceptual_caption_val_0": (caption_shard, 4, 13),
    "vqav2_train": (vqa_shard, 4, 14), "vqav2_trainable_val": (vqa_shard, 3, 15), "vqav2_val": (vqa_shard, 4, 16), "vqav2_rest_val": (vqa_shard, 2, 17),
    "nlvr2_train": (nlvr2_shard, 5, 18), "nlvr2_dev": (nlvr2_shard, 3, 19), "nlvr2_test1": (nlvr2_shard, 2, 20),
}


def write_toy_root(root: str, only=None) -> str:
    os.makedirs(root, exist_ok=True)
    for name, (writer, n, seed) in SHARDS.items():
        if only is None or name.startswith(tuple(only)):
            writer(os.path.join(root, name + ".arrow"), n, seed)
    return root


def toy_config(task, root, **over):
    """a task config on the toy root: 2 layers, 64-pixel images (MinMaxResize(64, 106): at most 96 x 128 after the resize), batch 4, no
    loader processes, the toy vocabulary"""
    kw = dict(data_root=root, tokenizer=VOCAB, num_layers=2, image_size=64, per_gpu_batchsize=4, batch_size=4, num_workers=0, max_steps=2,
              warmup_steps=0, drop_rate=0.0, max_image_len=-1, num_gpus=1, num_nodes=1, val_check_interval=1.0)
    kw.update(over)
    return task(**kw)
