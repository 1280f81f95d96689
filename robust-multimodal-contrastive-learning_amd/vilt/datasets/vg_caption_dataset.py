"""Visual Genome region captions (reference vilt/datasets/vg_caption_dataset.py): one training table "vg"; the val and test splits are
empty (pre-training validates on the other datasets of the recipe)."""
from __future__ import annotations

from .base_dataset import BaseDataset

SPLIT_NAMES = {"train": ["vg"], "val": [], "test": []}


class VisualGenomeCaptionDataset(BaseDataset):
    def __init__(self, *args, split="", **kwargs):
        assert split in SPLIT_NAMES, split
        self.split = split
        super().__init__(*args, **kwargs, names=SPLIT_NAMES[split], text_column_name="caption")
