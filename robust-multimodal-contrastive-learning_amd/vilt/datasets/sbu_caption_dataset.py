"""SBU captions (reference vilt/datasets/sbu_caption_dataset.py): nine training tables sbu_0 .. sbu_8; the val and test splits are empty."""
from __future__ import annotations

from .base_dataset import BaseDataset

SPLIT_NAMES = {"train": [f"sbu_{i}" for i in range(9)], "val": [], "test": []}


class SBUCaptionDataset(BaseDataset):
    def __init__(self, *args, split="", **kwargs):
        assert split in SPLIT_NAMES, split
        self.split = split
        super().__init__(*args, **kwargs, names=SPLIT_NAMES[split], text_column_name="caption")
