from ..datasets import VisualGenomeCaptionDataset
from .datamodule_base import BaseDataModule


class VisualGenomeCaptionDataModule(BaseDataModule):
    @property
    def dataset_cls(self):
        return VisualGenomeCaptionDataset

    @property
    def dataset_name(self):
        return "vg"
