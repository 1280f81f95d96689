"""COCO captions, Karpathy split (reference vilt/datasets/coco_caption_karpathy_dataset.py).  Shards: train = the train and restval
tables; val and test both read the TEST table (the reference validates on it).  On the test split every sample carries ``iid``, the
integer in the file name of its ``image_id`` ("COCO_val2014_000000391895.jpg" -> 391895)."""
from __future__ import annotations

from .base_dataset import BaseDataset

SPLIT_NAMES = {"train": ["coco_caption_karpathy_train", "coco_caption_karpathy_restval"], "val": ["coco_caption_karpathy_test"],
               "test": ["coco_caption_karpathy_test"]}


class CocoCaptionKarpathyDataset(BaseDataset):
    def __init__(self, *args, split="", **kwargs):
        assert split in SPLIT_NAMES, split
        self.split = split
        super().__init__(*args, **kwargs, names=SPLIT_NAMES[split], text_column_name="caption")

    def __getitem__(self, index):
        sample = self.get_suite(index)
        if "test" in self.split:
            row, _ = self.index_mapper[index]
            name = self.table["image_id"][row].as_py()
            sample["iid"] = int(name.split(".")[0].split("_")[-1])
        return sample
