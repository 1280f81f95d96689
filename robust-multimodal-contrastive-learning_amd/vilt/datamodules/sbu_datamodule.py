from ..datasets import SBUCaptionDataset
from .datamodule_base import BaseDataModule


class SBUCaptionDataModule(BaseDataModule):
    @property
    def dataset_cls(self):
        return SBUCaptionDataset

    @property
    def dataset_name(self):
        return "sbu"
