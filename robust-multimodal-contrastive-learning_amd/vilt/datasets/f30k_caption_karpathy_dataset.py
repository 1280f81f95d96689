"""Flickr30k captions, Karpathy split (reference vilt/datasets/f30k_caption_karpathy_dataset.py).  Shards: train = the train and val
tables; val and test both read the TEST table."""
from __future__ import annotations

from .base_dataset import BaseDataset

SPLIT_NAMES = {"train": ["f30k_caption_karpathy_train", "f30k_caption_karpathy_val"], "val": ["f30k_caption_karpathy_test"],
               "test": ["f30k_caption_karpathy_test"]}


class F30KCaptionKarpathyDataset(BaseDataset):
    def __init__(self, *args, split="", **kwargs):
        assert split in SPLIT_NAMES, split
        self.split = split
        super().__init__(*args, **kwargs, names=SPLIT_NAMES[split], text_column_name="caption")
