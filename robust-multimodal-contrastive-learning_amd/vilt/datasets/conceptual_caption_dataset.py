"""Conceptual Captions (reference vilt/datasets/conceptual_caption_dataset.py): training tables conceptual_caption_train_0 .. _28 (the
reference reads 29 of them), val and test both read conceptual_caption_val_0."""
from __future__ import annotations

from .base_dataset import BaseDataset

SPLIT_NAMES = {"train": [f"conceptual_caption_train_{i}" for i in range(29)], "val": ["conceptual_caption_val_0"],
               "test": ["conceptual_caption_val_0"]}


class ConceptualCaptionDataset(BaseDataset):
    def __init__(self, *args, split="", **kwargs):
        assert split in SPLIT_NAMES, split
        self.split = split
        super().__init__(*args, **kwargs, names=SPLIT_NAMES[split], text_column_name="caption")
