"""``MTDataModule(config, dist)``: the datamodules of ``config["datasets"]`` concatenated (reference multitask_datamodule.py, without
Lightning).  One ``collate`` for all of them, bound to the first datamodule's masked-LM collator; ``DistributedSampler``s when
``dist``.  Like the reference's, the validation sampler of a distributed run shuffles (each rank validates on its own shard either way;
the epoch metrics do not depend on the order); without ``dist`` no loader shuffles, as there."""
from __future__ import annotations

import functools

from torch.utils.data import DataLoader
from torch.utils.data.dataset import ConcatDataset
from torch.utils.data.distributed import DistributedSampler

DEFAULT_DATASETS = ["coco", "vg", "sbu", "gcc"]          # the reference config's default


class MTDataModule:
    def __init__(self, _config, dist=False):
        from . import _datamodules
        datamodule_keys = _config.get("datasets", DEFAULT_DATASETS)
        assert len(datamodule_keys) > 0
        unknown = [k for k in datamodule_keys if k not in _datamodules]
        if unknown:
            raise KeyError(f"config['datasets'] names {unknown}; known: {sorted(_datamodules)}")
        self.dm_keys = datamodule_keys
        self.dm_dicts = {key: _datamodules[key](_config) for key in datamodule_keys}
        self.dms = [v for k, v in self.dm_dicts.items()]
        self.batch_size = self.dms[0].batch_size
        self.vocab_size = self.dms[0].vocab_size
        self.num_workers = self.dms[0].num_workers
        self.dist = dist

    def prepare_data(self):
        pass

    def setup(self, stage=None):
        for dm in self.dms:
            dm.setup(stage)
        self.train_dataset = ConcatDataset([dm.train_dataset for dm in self.dms])
        self.val_dataset = ConcatDataset([dm.val_dataset for dm in self.dms])
        self.test_dataset = ConcatDataset([dm.test_dataset for dm in self.dms])
        self.tokenizer = self.dms[0].tokenizer
        self.collate = functools.partial(self.dms[0].train_dataset.collate, mlm_collator=self.dms[0].mlm_collator)
        if self.dist:
            self.train_sampler = DistributedSampler(self.train_dataset, shuffle=True)
            self.val_sampler = DistributedSampler(self.val_dataset, shuffle=True)
            self.test_sampler = DistributedSampler(self.test_dataset, shuffle=False)
        else:
            self.train_sampler = self.val_sampler = self.test_sampler = None

    def _loader(self, dataset, sampler, batch_size=None):
        return DataLoader(dataset, batch_size=batch_size if batch_size is not None else self.batch_size, sampler=sampler,
                          num_workers=self.num_workers, collate_fn=self.collate)

    def train_dataloader(self):
        return self._loader(self.train_dataset, self.train_sampler)

    def val_dataloader(self, batch_size=None):
        return self._loader(self.val_dataset, self.val_sampler, batch_size)

    def test_dataloader(self):
        return self._loader(self.test_dataset, self.test_sampler)
