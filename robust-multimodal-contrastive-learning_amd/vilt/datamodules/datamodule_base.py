"""``BaseDataModule(config)``: the three datasets of one corpus, their loaders, the tokenizer and the masked-LM collator (behaviour of
the reference's vilt/datamodules/datamodule_base.py, without Lightning).

What differs from the reference, on purpose (INTEGRATION.md "Datamodules"):
  * the tokenizer comes from ``attack.word_substitution.load_tokenizer(config["tokenizer"])`` - a tokenizer object, or a local
    vocabulary (a ``vocab.txt`` or the directory holding it).  A name that is not on disk is an error; nothing is fetched;
  * ``mlm_collator`` is ``masking_collator`` with the tokenizer's ids (whole-word masking when ``config["whole_word_masking"]``);
  * ``config.get("image_feed", "device")``: "device" puts the recipe on the byte feed - the transform keys "pixelbert" and
    "pixelbert_randaug" become "decode_uint8" and "decode_uint8_randaug" (workers only decode; RandAugment, MinMaxResize and the
    normalisation run on the device) -, "host" leaves the keys as the config has them."""
from __future__ import annotations

import torch
from torch.utils.data import DataLoader

from ..datasets.base_dataset import masking_collator

DEVICE_FEED = {"pixelbert": "decode_uint8", "pixelbert_randaug": "decode_uint8_randaug"}
DEFAULT_TRANSFORM_KEYS = ["pixelbert"]                   # the reference config's default for both splits


def get_local_tokenizer(spec):
    """config["tokenizer"] -> a tokenizer, from this machine only"""
    from ...attack.word_substitution import load_tokenizer
    tok = load_tokenizer(spec)
    if tok is None:
        raise FileNotFoundError(f"config['tokenizer'] = {spec!r} is neither a tokenizer object nor a local vocabulary (a vocab.txt or the "
                                "directory holding it); hub names such as 'bert-base-uncased' are not fetched - point it at a local copy")
    return tok


def feed_keys(keys, feed: str):
    if feed not in ("device", "host"):
        raise ValueError(f"config['image_feed'] must be 'device' or 'host' (got {feed!r})")
    keys = list(keys) if len(keys) else list(DEFAULT_TRANSFORM_KEYS)
    return [DEVICE_FEED.get(k, k) for k in keys] if feed == "device" else keys


def continuation_ids_of(tokenizer):
    """ids of the vocabulary's ## pieces (whole-word masking)"""
    return sorted(i for t, i in tokenizer.get_vocab().items() if t.startswith("##"))


class BaseDataModule:
    def __init__(self, _config):
        self.data_dir = _config["data_root"]
        self.num_workers = _config["num_workers"]
        self.batch_size = _config["per_gpu_batchsize"]
        self.eval_batch_size = self.batch_size
        self.image_size = _config["image_size"]
        self.max_text_len = _config["max_text_len"]
        self.draw_false_image = _config["draw_false_image"]
        self.draw_false_text = _config["draw_false_text"]
        self.image_only = _config["image_only"]
        self.image_feed = _config.get("image_feed", "device")
        self.train_transform_keys = feed_keys(_config.get("train_transform_keys", ()), self.image_feed)
        self.val_transform_keys = feed_keys(_config.get("val_transform_keys", ()), self.image_feed)
        self.tokenizer = get_local_tokenizer(_config["tokenizer"])
        self.vocab_size = self.tokenizer.vocab_size
        tok = self.tokenizer
        wwm = bool(_config["whole_word_masking"])
        self.mlm_collator = masking_collator(
            tok.mask_token_id, self.vocab_size, special_ids=tok.all_special_ids, mlm_prob=_config["mlm_prob"], max_text_len=self.max_text_len,
            pad_id=tok.pad_token_id, whole_word_masking=wwm, continuation_ids=continuation_ids_of(tok) if wwm else None)
        self.setup_flag = False

    @property
    def dataset_cls(self):
        raise NotImplementedError("a datamodule names its dataset class")

    @property
    def dataset_name(self):
        raise NotImplementedError("a datamodule names its key of the _datamodules table")

    def _make(self, cls, keys, split, **over):
        kw = dict(image_size=self.image_size, max_text_len=self.max_text_len, draw_false_image=self.draw_false_image,
                  draw_false_text=self.draw_false_text, image_only=self.image_only)
        kw.update(over)
        return cls(self.data_dir, keys, split=split, **kw)

    def set_train_dataset(self):
        self.train_dataset = self._make(self.dataset_cls, self.train_transform_keys, "train")

    def set_val_dataset(self):
        self.val_dataset = self._make(self.dataset_cls, self.val_transform_keys, "val")
        if hasattr(self, "dataset_cls_no_false"):
            self.val_dataset_no_false = self._make(self.dataset_cls_no_false, self.val_transform_keys, "val", draw_false_image=0, draw_false_text=0)

    def make_no_false_val_dset(self, image_only=False, max_num=-1):
        return self._make(self.dataset_cls_no_false, self.val_transform_keys, "val", draw_false_image=0, draw_false_text=0,
                          image_only=image_only, max_num=max_num)

    def set_test_dataset(self):
        self.test_dataset = self._make(self.dataset_cls, self.val_transform_keys, "test")

    def setup(self, stage=None):
        if not self.setup_flag:
            self.set_train_dataset()
            self.set_val_dataset()
            self.set_test_dataset()
            self.train_dataset.tokenizer = self.tokenizer
            self.val_dataset.tokenizer = self.tokenizer
            self.test_dataset.tokenizer = self.tokenizer
            self.setup_flag = True

    def _loader(self, dataset, batch_size, shuffle):
        return DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=self.num_workers, pin_memory=torch.cuda.is_available(),
                          collate_fn=dataset.collate)

    def train_dataloader(self):
        return self._loader(self.train_dataset, self.batch_size, True)

    def val_dataloader(self):
        return self._loader(self.val_dataset, self.eval_batch_size, False)

    def test_dataloader(self):
        return self._loader(self.test_dataset, self.eval_batch_size, False)
