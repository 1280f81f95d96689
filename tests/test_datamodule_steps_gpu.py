"""-m gpu: ``Trainer(config).run(model)`` WITHOUT loaders - the datamodule of the config builds them from a toy ``data_root``
(tests/datamodule_toy.py) on the device feed (``image_feed="device"``: workers only decode) - for one recipe of every family: two
optimizer steps, one validation pass, and what the model reads through ``model.trainer.datamodule``.  Two-layer models, 64-pixel images
(at most 96 x 128 after MinMaxResize), batch 4, ``num_workers=0``: no loader process is forked after the GPU is open.

The first-step loss of ``task_mlm_itm_mpp`` and ``task_finetune_vqa`` on the device feed against the host feed follows the rule of
tests/test_feed_gpu.py (test_training_step_on_a_byte_batch_equals_the_float_batch): both feeds hand the encoder identical patch rows,
so |loss_a - loss_b| <= 1e-6 |loss_a| (the order of the float atomics of the batch loss)."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd.trainer import Trainer, to_device  # noqa: E402
from rmcl_amd.vilt import config as C  # noqa: E402
from rmcl_amd.vilt.datamodules import MTDataModule  # noqa: E402
from rmcl_amd.vilt.datasets import RawUint8Batch  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from tests.datamodule_toy import toy_config, write_toy_root  # noqa: E402

DEV = "cuda:0"

RECIPES = {
    "task_mlm_itm_mpp": {},
    "task_finetune_vqa_randaug": {},
    "task_finetune_nlvr2": {},
    "task_finetune_irtr_coco": {},
    "task_moco": dict(datasets=["coco"], image_view=True, num_negative=1024, adv_steps_img=2),
}


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return write_toy_root(str(tmp_path_factory.mktemp("toy_root")))


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_trainer_runs_a_recipe_from_its_config_and_a_data_root(root, recipe, tmp_path):
    cfg = toy_config(getattr(C, recipe), root, image_feed="device", max_steps=2, val_check_interval=2, log_dir=str(tmp_path), **RECIPES[recipe])
    torch.manual_seed(0)
    random.seed(0)
    model = ViLTransformerSS(cfg, device=DEV, compute_dtype="bf16")
    before = model.engine.q32.clone()
    losses, feeds = [], []
    step = model.training_step

    def recording_step(batch, idx):
        feeds.append(type(batch[[k for k in batch if "image" in k][0]][0]))
        loss = step(batch, idx)
        losses.append(float(loss.detach()))
        return loss
    model.training_step = recording_step
    tr = Trainer(cfg, ckpt_dir=str(tmp_path / "ckpt"))
    tr.run(model)
    torch.cuda.synchronize()
    assert tr.global_step == 2 and len(losses) == 2 and all(math.isfinite(v) for v in losses), losses
    assert feeds == [RawUint8Batch, RawUint8Batch]                                     # the device feed: decoded bytes reach the step
    assert not torch.equal(model.engine.q32, before) and bool(torch.isfinite(model.engine.q32).all())
    assert isinstance(tr.datamodule, MTDataModule) and model.trainer is tr and list(tr.datamodule.dm_dicts) == cfg["datasets"]
    assert tr.validations == 1
    metrics = model.last_epoch_metrics
    assert metrics["phase"] == "val" and len(metrics) > 1
    for k, v in metrics.items():
        if isinstance(v, float) and not k.endswith("accuracy") and "accuracy" not in k:
            assert math.isfinite(v), (k, v)
    if recipe == "task_finetune_irtr_coco":
        recalls = [metrics[f"recalls/{n}"] for n in ("ir_r1", "ir_r5", "ir_r10", "tr_r1", "tr_r5", "tr_r10")]   # through model.trainer.datamodule
        assert all(0.0 <= r <= 1.0 for r in recalls)                                   # 12 images x 24 captions of the toy validation split
        assert recalls[0] <= recalls[1] <= recalls[2] and recalls[3] <= recalls[4] <= recalls[5] and recalls[2] > 0 and recalls[5] > 0
    if recipe == "task_finetune_vqa_randaug":
        vqa = tr.datamodule.dm_dicts["vqa"]
        assert model.id2answer is vqa.id2answer and model.id2answer[0] == "yes" and vqa.num_class == 7
    if recipe == "task_mlm_itm_mpp":
        assert set(model.current_tasks) == {"itm", "mlm", "mpp"}


@pytest.mark.parametrize("recipe", ["task_mlm_itm_mpp", "task_finetune_vqa"])
def test_first_step_loss_on_the_device_feed_equals_the_host_feed(root, recipe):
    torch.manual_seed(0)
    model = ViLTransformerSS(toy_config(getattr(C, recipe), root), device=DEV, compute_dtype="bf16")
    model.train()
    got = {}
    for feed in ("host", "device"):
        dm = MTDataModule(toy_config(getattr(C, recipe), root, image_feed=feed))
        dm.setup("fit")
        random.seed(5)                                                  # false-image draws of the samples
        torch.manual_seed(5)                                            # the collator's masks; then the step's own draws (ITM labels, MPP masks)
        batch = next(iter(dm.train_dataloader()))
        view = batch["image"][0]
        assert isinstance(view, RawUint8Batch) if feed == "device" else torch.is_tensor(view)
        model.zero_grad()
        loss = model.training_step(to_device(batch, model.device), 0)
        loss.backward()
        torch.cuda.synchronize()
        got[feed] = (float(loss.detach()), tuple(view.shape), batch["text_ids"].clone())
    assert got["host"][1] == got["device"][1] and torch.equal(got["host"][2], got["device"][2])      # the same samples
    print(recipe, "first-step loss host", got["host"][0], "device", got["device"][0])
    assert math.isfinite(got["host"][0]) and abs(got["host"][0] - got["device"][0]) <= 1e-6 * abs(got["host"][0])
