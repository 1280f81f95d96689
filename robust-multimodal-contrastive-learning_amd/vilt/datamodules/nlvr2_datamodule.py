from ..datasets import NLVR2Dataset
from .datamodule_base import BaseDataModule


class NLVR2DataModule(BaseDataModule):
    @property
    def dataset_cls(self):
        return NLVR2Dataset

    @property
    def dataset_name(self):
        return "nlvr2"
