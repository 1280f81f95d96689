"""VQAv2 (reference vilt/datasets/vqav2_dataset.py): one sample = an image and ONE of its questions (column "questions", duplicates kept:
the question number indexes the answer columns) with ``qid`` (column "question_id") and, outside the test split, the answers of that
question: ``vqa_answer`` (strings), ``vqa_labels`` (class ids) and ``vqa_scores`` (soft scores) from the columns "answers",
"answer_labels" and "answer_scores"; on the test split the three are empty lists.  Shards: train = vqav2_train + vqav2_trainable_val,
val and test both read vqav2_val."""
from __future__ import annotations

from .base_dataset import BaseDataset

SPLIT_NAMES = {"train": ["vqav2_train", "vqav2_trainable_val"], "val": ["vqav2_val"], "test": ["vqav2_val"]}


class VQAv2Dataset(BaseDataset):
    def __init__(self, *args, split="", **kwargs):
        assert split in SPLIT_NAMES, split
        self.split = split
        super().__init__(*args, **kwargs, names=SPLIT_NAMES[split], text_column_name="questions", remove_duplicate=False)

    def __getitem__(self, index):
        sample = {"image": self.get_image(index)["image"], "text": self.get_text(index)["text"]}
        row, q = self.index_mapper[index]
        cell = lambda column: self.table[column][row][q].as_py()
        labelled = self.split != "test"
        sample.update(vqa_answer=cell("answers") if labelled else [], vqa_labels=cell("answer_labels") if labelled else [],
                      vqa_scores=cell("answer_scores") if labelled else [], qid=cell("question_id"))
        return sample
