"""NLVR2 pairs (reference vilt/datasets/nlvr2_dataset.py): one sample = two images of one row (columns "image_0" / "image_1"), one of
its statements (column "questions") and its label (column "answers", the strings "True" / "False" -> bool).  Shards: nlvr2_train for
the train split, nlvr2_dev + nlvr2_test1 for val and test; ``table_name`` tells the dev rows from the test rows
(compute_nlvr2's separate logs).  ``collate`` pads image_0 and image_1 of a batch to one shared extent."""
from __future__ import annotations

from .base_dataset import BaseDataset

SPLIT_NAMES = {"train": ["nlvr2_train"], "val": ["nlvr2_dev", "nlvr2_test1"], "test": ["nlvr2_dev", "nlvr2_test1"]}


class NLVR2Dataset(BaseDataset):
    def __init__(self, *args, split="", **kwargs):
        assert split in SPLIT_NAMES, split
        self.split = split
        super().__init__(*args, **kwargs, names=SPLIT_NAMES[split], text_column_name="questions", remove_duplicate=False)

    def _pair(self, index) -> dict:
        image_0 = self.get_image(index, image_key="image_0")["image"]
        image_1 = self.get_image(index, image_key="image_1")["image"]
        text = self.get_text(index)["text"]
        row, q = self.index_mapper[index]
        return {"image_0": image_0, "image_1": image_1, "text": text, "answers": self.table["answers"][row][q].as_py() == "True",
                "table_name": self.table_names[row]}

    def __getitem__(self, index):
        """a record that cannot be read is reported and replaced by a randomly drawn one (nlvr2_dataset.py:29-40)"""
        entry = index
        while True:
            try:
                return self._pair(entry)
            except Exception as err:
                print(f"[NLVR2Dataset] entry {entry} of {self.names[0]} could not be loaded ({type(err).__name__}: {err}); drawing another sample")
                entry = self._any_entry()
