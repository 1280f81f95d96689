"""CPU: the dataset classes of every recipe (rmcl_amd.vilt.datasets), the datamodules (rmcl_amd.vilt.datamodules) and ``MTDataModule`` on
a toy ``data_root`` (tests/datamodule_toy.py), against the shard names of the reference's classes and against what the reference's own
``CocoCaptionKarpathyDataset`` / ``VQAv2Dataset`` gave on the same shards (tests/golden/datamodules.json, tools/gen_golden_datamodules.py)."""
import json
import os
import random

import pytest
import torch

import rmcl_pkg  # noqa: F401
from rmcl_amd.vilt import config as C
from rmcl_amd.vilt import datasets as D
from rmcl_amd.vilt.datamodules import MTDataModule, _datamodules
from rmcl_amd.vilt.datasets import RawUint8Batch
from tests.datamodule_toy import SHARDS, VOCAB, toy_config, write_toy_root

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datamodules.json")

# class -> split -> the shard names, literally (the on-disk contract of data_root)
NAMES = {
    "CocoCaptionKarpathyDataset": {"train": ["coco_caption_karpathy_train", "coco_caption_karpathy_restval"], "val": ["coco_caption_karpathy_test"],
                                   "test": ["coco_caption_karpathy_test"]},
    "F30KCaptionKarpathyDataset": {"train": ["f30k_caption_karpathy_train", "f30k_caption_karpathy_val"], "val": ["f30k_caption_karpathy_test"],
                                   "test": ["f30k_caption_karpathy_test"]},
    "VisualGenomeCaptionDataset": {"train": ["vg"], "val": [], "test": []},
    "SBUCaptionDataset": {"train": [f"sbu_{i}" for i in range(9)], "val": [], "test": []},
    "ConceptualCaptionDataset": {"train": [f"conceptual_caption_train_{i}" for i in range(29)], "val": ["conceptual_caption_val_0"],
                                 "test": ["conceptual_caption_val_0"]},
    "VQAv2Dataset": {"train": ["vqav2_train", "vqav2_trainable_val"], "val": ["vqav2_val"], "test": ["vqav2_val"]},
    "NLVR2Dataset": {"train": ["nlvr2_train"], "val": ["nlvr2_dev", "nlvr2_test1"], "test": ["nlvr2_dev", "nlvr2_test1"]},
}
CAPTION_KEYS = {"image", "text", "img_index", "cap_index", "raw_index", "replica"}


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return write_toy_root(str(tmp_path_factory.mktemp("toy_root")))


@pytest.fixture(scope="module")
def tok():
    from rmcl_amd.attack.word_substitution import load_tokenizer
    return load_tokenizer(VOCAB)


def _captions_of(root, names, column):
    """(captions per image row, rows) of the named shards that exist, read with pyarrow alone"""
    import pyarrow as pa
    out = []
    for n in names:
        p = os.path.join(root, n + ".arrow")
        if os.path.isfile(p):
            out += pa.ipc.RecordBatchFileReader(pa.memory_map(p, "r")).read_all()[column].to_pylist()
    return out


@pytest.mark.parametrize("split", ["train", "val", "test"])
@pytest.mark.parametrize("cls", sorted(NAMES))
def test_dataset_shards_length_index_and_sample_keys(root, tok, cls, split):
    klass = getattr(D, cls)
    ds = klass(root, ["pixelbert"], split=split, image_size=64, max_text_len=40, draw_false_image=0, draw_false_text=0, image_only=False)
    ds.tokenizer = tok
    assert ds.names == NAMES[cls][split]
    dedup = cls not in ("VQAv2Dataset", "NLVR2Dataset")
    column = "caption" if dedup else "questions"
    texts = _captions_of(root, ds.names, column)
    counts = [len(dict.fromkeys(t)) if dedup else len(t) for t in texts]
    assert len(ds) == sum(counts)
    assert [n for n in ds.names if n in SHARDS] == list(dict.fromkeys(ds.table_names)) if counts else ds.table is None
    if not counts:
        assert len(ds) == 0 and ds.index_mapper == {}
        return
    assert ds.index_mapper[0] == (0, 0) and ds.index_mapper[len(ds) - 1] == (len(counts) - 1, counts[-1] - 1)
    first, last = ds[0], ds[len(ds) - 1]
    for s in (first, last):
        if cls == "VQAv2Dataset":
            assert set(s) == {"image", "text", "vqa_answer", "vqa_labels", "vqa_scores", "qid"}
            if split == "test":
                assert s["vqa_answer"] == [] and s["vqa_labels"] == [] and s["vqa_scores"] == []
            else:
                assert len(s["vqa_answer"]) == len(s["vqa_labels"]) == len(s["vqa_scores"]) >= 1
        elif cls == "NLVR2Dataset":
            assert set(s) == {"image_0", "image_1", "text", "answers", "table_name"}
        elif cls == "CocoCaptionKarpathyDataset" and split == "test":
            assert set(s) == CAPTION_KEYS | {"iid"} and isinstance(s["iid"], int)
        else:
            assert set(s) == CAPTION_KEYS
    assert first["text"][0] == list(dict.fromkeys(texts[0]))[0] if dedup else texts[0][0]
    if cls == "CocoCaptionKarpathyDataset" and split == "test":
        assert first["iid"] == 3000 and last["iid"] == 3011              # "COCO_val2014_000000003000.jpg" -> 3000


def test_vg_and_sbu_and_gcc_test_split_is_the_val_split(root):
    for cls in ("VisualGenomeCaptionDataset", "SBUCaptionDataset", "ConceptualCaptionDataset"):
        a = getattr(D, cls)(root, ["pixelbert"], split="val", image_size=64)
        b = getattr(D, cls)(root, ["pixelbert"], split="test", image_size=64)
        assert a.names == b.names and len(a) == len(b)
    with pytest.raises(AssertionError):
        D.VQAv2Dataset(root, ["pixelbert"], split="dev", image_size=64)


@pytest.mark.parametrize("split", ["train", "val", "test"])
@pytest.mark.parametrize("key", ["coco", "vqa"])
def test_datasets_against_the_references_own_classes(root, tok, key, split):
    gold = json.load(open(GOLD))
    rec = gold[f"{key}_{split}"]
    klass = D.CocoCaptionKarpathyDataset if key == "coco" else D.VQAv2Dataset
    ds = klass(root, ["pixelbert"], split=split, image_size=gold["image_size"], max_text_len=40, draw_false_image=0,
               draw_false_text=gold["draw_false_text"] if key == "coco" else 0, image_only=False)
    ds.tokenizer = tok
    assert list(ds.names) == rec["names"] and len(ds) == rec["len"]
    ent = lambda j: [ds.index_mapper[j][0], -1 if ds.index_mapper[j][1] is None else ds.index_mapper[j][1]]
    assert ent(0) == rec["first"] and ent(len(ds) - 1) == rec["last"]
    random.seed(gold["seed"])                                             # the generator drew its samples in this order under this seed
    for j in sorted(int(k) for k in rec["samples"]):
        want, s = rec["samples"][str(j)], ds[j]
        assert sorted(s.keys()) == want["keys"]
        if key == "coco":
            # the reference's caption order inside an image depends on the hash seed (list(set(...))): order-free facts
            assert [int(s["img_index"]), int(s["cap_index"]), int(s["raw_index"]), int(s["replica"])] == want["meta"]
            assert sorted(ds.all_texts[s["img_index"]]) == want["row_captions"] and s["text"][0] in want["row_captions"]
            for r, row in enumerate(want["false_rows"]):                  # the same draws from `random` land in the same image rows
                text = s[f"false_text_{r}"][0]
                mine = next(caps for caps in ds.all_texts if text in caps)
                assert sorted(mine) == row
            if "iid" in want:
                assert s["iid"] == want["iid"]
        else:
            assert s["text"][0] == want["text"] and list(s["text"][1]["input_ids"]) == want["ids"]
            assert s["vqa_answer"] == want["vqa_answer"] and s["vqa_labels"] == want["vqa_labels"] and s["vqa_scores"] == want["vqa_scores"]
            assert s["qid"] == want["qid"] and list(s["image"][0].shape) == want["image_shape"]


# ---- datamodules ---------------------------------------------------------------------------------------------------------------------
def test_key_table():
    assert sorted(_datamodules) == sorted(["coco", "f30k", "vg", "sbu", "gcc", "vqa", "nlvr2"])
    for k, cls in _datamodules.items():
        assert cls.dataset_name.fget(object.__new__(cls)) == k


def test_vqa_datamodule_reads_the_answer_vocabulary(root):
    cfg = toy_config(C.task_finetune_vqa, root)
    dm = MTDataModule(cfg)
    dm.setup("fit")
    vqa = dm.dm_dicts["vqa"]
    from tests.datamodule_toy import ANSWERS
    seen = {}
    for n in ("vqav2_train", "vqav2_trainable_val", "vqav2_val"):
        for per_image_a, per_image_l in zip(_captions_of(root, [n], "answers"), _captions_of(root, [n], "answer_labels")):
            for qa, ql in zip(per_image_a, per_image_l):
                seen.update(zip(qa, ql))
    assert vqa.answer2id == seen and vqa.num_class == max(seen.values()) + 1
    for a, i in seen.items():
        assert vqa.id2answer[i] == a == ANSWERS[i]
    assert vqa.id2answer[10 ** 6] == "unknown"
    assert len(dm.test_dataset) == len(dm.val_dataset) > 0


def test_make_no_false_val_dset(root):
    dm = MTDataModule(toy_config(C.task_finetune_irtr_coco, root))
    dm.setup("fit")
    coco = dm.dms[0]
    img = coco.make_no_false_val_dset(image_only=True, max_num=3)
    assert len(img) == 3 and [img.index_mapper[i] for i in range(3)] == [(0, None), (1, None), (2, None)]
    img.tokenizer = coco.tokenizer
    assert "text" not in img[0] and "false_text_0" not in img[0]
    txt = coco.make_no_false_val_dset(max_num=2)
    assert len(txt) == sum(len(t) for t in txt.all_texts[:2]) and txt.draw_false_text == 0 and txt.draw_false_image == 0
    assert coco.val_dataset.draw_false_text == 15 and coco.val_dataset_no_false.draw_false_text == 0


def test_mt_datamodule_concatenates_and_binds_the_first_collator(root):
    cfg = toy_config(C.task_mlm_itm_mpp, root)
    assert cfg["datasets"] == ["coco", "vg", "sbu", "gcc"]
    dm = MTDataModule(cfg, dist=False)
    dm.setup("fit")
    assert [d.dataset_name for d in dm.dms] == cfg["datasets"] and list(dm.dm_dicts) == cfg["datasets"]
    assert len(dm.train_dataset) == sum(len(d.train_dataset) for d in dm.dms) and len(dm.train_dataset) > len(dm.dms[0].train_dataset)
    assert len(dm.val_dataset) == len(dm.dms[0].val_dataset) + len(dm.dm_dicts["gcc"].val_dataset)
    assert dm.collate.keywords["mlm_collator"] is dm.dms[0].mlm_collator and dm.tokenizer is dm.dms[0].tokenizer
    assert dm.train_sampler is None and dm.vocab_size == 1148 and dm.batch_size == 4
    two = MTDataModule(toy_config(C.task_mlm_itm, root, datasets=["coco", "f30k"]))
    two.setup("fit")
    assert len(two.train_dataset) == len(two.dms[0].train_dataset) + len(two.dms[1].train_dataset)
    assert two.collate.keywords["mlm_collator"] is two.dms[0].mlm_collator


RECIPE_KEYS = {
    "task_mlm_itm_mpp": ["image", "false_image_0", "text_ids", "text_masks", "text_ids_mlm", "text_labels_mlm", "text_labels"],
    "task_finetune_vqa_randaug": ["image", "text_ids", "text_masks", "vqa_labels", "vqa_scores", "vqa_answer", "qid"],
    "task_finetune_nlvr2": ["image_0", "image_1", "text_ids", "text_masks", "answers", "table_name"],
    "task_finetune_irtr_coco": ["image", "text_ids", "text_masks", "false_image_0"] + [f"false_text_{i}_ids" for i in range(15)]
                               + [f"false_text_{i}_masks" for i in range(15)],
    "task_moco": ["image", "text_ids", "text_masks", "text"],
}


@pytest.mark.parametrize("recipe", sorted(RECIPE_KEYS))
def test_collated_batches_and_the_image_feed(root, recipe):
    over = {"datasets": ["coco"]} if recipe == "task_moco" else {}
    for feed in ("device", "host"):
        random.seed(3)
        torch.manual_seed(3)
        dm = MTDataModule(toy_config(getattr(C, recipe), root, image_feed=feed, **over))
        dm.setup("fit")
        batch = next(iter(dm.train_dataloader()))
        for k in RECIPE_KEYS[recipe]:
            assert k in batch, (k, sorted(batch))
        assert tuple(batch["text_ids"].shape) == (4, 40)
        image_keys = [k for k in batch if "image" in k]
        for k in image_keys:
            view = batch[k][0]
            if feed == "device":
                assert isinstance(view, RawUint8Batch) and view.data.dtype == torch.uint8 and view.shape[0] == 4
                assert (view.aug is not None) == ("randaug" in recipe)                     # plans travel with the _randaug recipes
                assert view.shape[2] % 32 == 0 and view.shape[3] % 32 == 0 and max(view.shape[2:]) <= 128
            else:
                assert torch.is_tensor(view) and view.dtype == torch.float32 and tuple(view.shape[:2]) == (4, 3)
        assert len({tuple(batch[k][0].shape) for k in image_keys}) == 1                      # one extent over all image keys
        val = next(iter(dm.val_dataloader()))
        vview = val[[k for k in val if "image" in k][0]][0]
        assert isinstance(vview, RawUint8Batch) and vview.aug is None if feed == "device" else torch.is_tensor(vview)
    if recipe == "task_mlm_itm_mpp":
        chosen = batch["text_labels_mlm"] != -100
        assert bool(((batch["text_ids_mlm"] == batch["text_ids"]) | chosen).all())


def test_transform_keys_of_the_two_feeds(root):
    dev = _datamodules["coco"](toy_config(C.task_finetune_irtr_coco_randaug, root))
    assert dev.train_transform_keys == ["decode_uint8_randaug"] and dev.val_transform_keys == ["decode_uint8"]
    host = _datamodules["coco"](toy_config(C.task_finetune_irtr_coco_randaug, root, image_feed="host"))
    assert host.train_transform_keys == ["pixelbert_randaug"] and host.val_transform_keys == ["pixelbert"]
    kept = _datamodules["coco"](toy_config(C.task_mlm_itm, root, train_transform_keys=["pixelbert_uint8"]))
    assert kept.train_transform_keys == ["pixelbert_uint8"]
    with pytest.raises(ValueError, match="image_feed"):
        _datamodules["coco"](toy_config(C.task_mlm_itm, root, image_feed="gpu"))


def test_an_unknown_tokenizer_name_is_an_error_and_nothing_is_fetched(root, monkeypatch):
    import socket

    def no_network(*a, **k):
        raise AssertionError("the datamodule tried to open a socket")
    monkeypatch.setattr(socket.socket, "connect", no_network)
    monkeypatch.setattr(socket, "create_connection", no_network)
    with pytest.raises(FileNotFoundError, match="bert-base-uncased"):
        MTDataModule(toy_config(C.task_mlm_itm, root, tokenizer="bert-base-uncased"))


def test_trainer_attaches_the_datamodule_once(root, tmp_path):
    import types
    from rmcl_amd.trainer import Trainer
    tr = Trainer(toy_config(C.task_finetune_vqa, root), ckpt_dir=str(tmp_path))
    assert tr.datamodule is None
    model = types.SimpleNamespace(id2answer=None)
    dm = tr.attach_datamodule(model)
    assert dm is tr.datamodule and isinstance(dm, MTDataModule) and dm.dist is False and model.trainer is tr
    assert model.id2answer is dm.dm_dicts["vqa"].id2answer and model.id2answer[1] == "no"
    assert tr.attach_datamodule(model) is dm                              # set up once
    other = types.SimpleNamespace(id2answer=None)
    Trainer(toy_config(C.task_mlm_itm, root), ckpt_dir=str(tmp_path)).attach_datamodule(other)
    assert other.id2answer is None and other.trainer.datamodule.dms[0].dataset_name == "coco"


def test_run_module_builds_its_config_from_the_command_line(root):
    from rmcl_amd.run import build_config
    cfg = build_config(["task_finetune_vqa_randaug", f"data_root={root}", "per_gpu_batchsize=4", "image_feed=host", "exp_name=toy", "learning_rate=2e-5",
                        "datasets=['vqa']"])
    assert cfg["train_transform_keys"] == ["pixelbert_randaug"] and cfg["loss_names"]["vqa"] == 1 and cfg["data_root"] == root
    assert cfg["per_gpu_batchsize"] == 4 and cfg["image_feed"] == "host" and cfg["exp_name"] == "toy" and cfg["learning_rate"] == 2e-5
    assert cfg["datasets"] == ["vqa"]
    assert build_config([])["loss_names"] == C.default_config()["loss_names"]
    with pytest.raises(SystemExit):
        build_config(["task_nothing"])
    with pytest.raises(SystemExit):
        build_config(["no_such_key=1"])


def test_whole_word_masking_collator_comes_from_the_vocabulary(root):
    dm = _datamodules["coco"](toy_config(C.task_mlm_itm, root, whole_word_masking=True, mlm_prob=0.3))
    tok = dm.tokenizer
    enc = tok("two dogs walking near the houses", truncation=True, max_length=40, padding="max_length")
    out = dm.mlm_collator([enc] * 8)
    pieces = tok.convert_ids_to_tokens(enc["input_ids"])
    chosen = out["labels"] != -100
    assert bool(chosen.any())
    for row in chosen:
        for t, p in enumerate(pieces):
            if p.startswith("##"):
                assert bool(row[t]) == bool(row[t - 1])                   # a ## piece goes with its word
