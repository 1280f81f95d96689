"""VQAv2: ``setup`` also reads the answer vocabulary off the shards (reference vqav2_datamodule.py:21-38): every (answer, label) pair of
the train and val tables' "answers" / "answer_labels" columns gives ``answer2id``; ``num_class`` = the largest label + 1;
``id2answer`` maps a label back to its string ("unknown" for a label no shard names) - what ``test_step`` writes out."""
from collections import defaultdict

from ..datasets import VQAv2Dataset
from .datamodule_base import BaseDataModule


def _unknown():
    return "unknown"


class VQAv2DataModule(BaseDataModule):
    @property
    def dataset_cls(self):
        return VQAv2Dataset

    @property
    def dataset_name(self):
        return "vqa"

    def setup(self, stage=None):
        super().setup(stage)
        pairs = {}
        for dset in (self.train_dataset, self.val_dataset):
            if dset.table is None:
                continue
            answers, labels = dset.table["answers"].to_pylist(), dset.table["answer_labels"].to_pylist()
            for per_image_a, per_image_l in zip(answers, labels):             # [question][answer] per image; None for an image without answers
                if per_image_a is None or per_image_l is None:
                    continue
                for qa, ql in zip(per_image_a, per_image_l):
                    pairs.update(zip(qa, ql))
        self.answer2id = pairs
        self.num_class = max(pairs.values()) + 1
        self.id2answer = defaultdict(_unknown)
        for answer, label in sorted(pairs.items(), key=lambda kv: kv[1]):
            self.id2answer[label] = answer
