from ..datasets import F30KCaptionKarpathyDataset
from .datamodule_base import BaseDataModule


class F30KCaptionKarpathyDataModule(BaseDataModule):
    @property
    def dataset_cls(self):
        return F30KCaptionKarpathyDataset

    @property
    def dataset_cls_no_false(self):
        return F30KCaptionKarpathyDataset

    @property
    def dataset_name(self):
        return "f30k"
