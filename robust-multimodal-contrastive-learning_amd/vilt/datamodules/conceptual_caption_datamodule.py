from ..datasets import ConceptualCaptionDataset
from .datamodule_base import BaseDataModule


class ConceptualCaptionDataModule(BaseDataModule):
    @property
    def dataset_cls(self):
        return ConceptualCaptionDataset

    @property
    def dataset_name(self):
        return "gcc"
