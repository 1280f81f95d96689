"""Rehearsal of the N > 1 code path of the mlm + itm + mpp step on ONE GPU (developer / test use, never a measurement): every rank of a
torch.distributed.run launch sits on cuda:0, gloo replaces RCCL (which refuses two ranks on one device).  Each rank runs --steps
optimizer steps on its OWN seeded batch and masks (2 layers, bf16, per-rank batch --batch); the three deferred backwards of a step meet
in one gradient reduction.  Prints one JSON line per launch (rank 0): `ranks_bit_identical` = the parameter arenas of all ranks hold the
same bits after the last step - the reference's DDP invariant.

  python -m torch.distributed.run --nproc-per-node 2 tools/mpp_two_rank.py --steps 2 --batch 4"""
import argparse
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.vilt.config import task_mlm_itm_mpp
    from rmcl_amd.vilt.modules import ViLTransformerSS
    from rmcl_amd.runtime import mpp_draw_masks
    from tools.mlm_bench import batch_of
    torch.manual_seed(0)                                                  # the same initial weights on every rank
    cfg = task_mlm_itm_mpp(num_layers=2, per_gpu_batchsize=a.batch, num_gpus=world, max_steps=100, warmup_steps=0, dense_images=True)
    m = ViLTransformerSS(cfg, device="cuda:0", compute_dtype="bf16")
    (opt,), _ = m.configure_optimizers()
    m.train()
    batch = batch_of(a.batch, cfg, "cuda:0", seed=100 + rank)             # another batch per rank
    torch.manual_seed(200 + rank)                                         # ... and other masks, dropout seeds aside
    batch["mpp_masked"], batch["mpp_replaced"] = mpp_draw_masks(a.batch, (cfg["image_size"] // cfg["patch_size"]) ** 2)
    loss = None
    for i in range(a.steps):
        m.zero_grad()
        loss = m.training_step(batch, i)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    q = m.engine.q32.detach().cpu()
    mine = torch.stack([q.double().sum(), q.double().abs().sum(), q.view(torch.int32).double().sum()])
    every = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    grads = m.engine.g32.detach().cpu()
    if rank == 0:
        print(json.dumps({"world_size": dist.get_world_size(), "steps": a.steps, "batch_per_rank": a.batch,
                          "ranks_bit_identical": all(torch.equal(e, every[0]) for e in every), "final_loss": float(loss),
                          "mpp_loss": float(m.logged["mpp/train/loss"]), "grad_abs_max": float(grads.abs().max()),
                          "mask_token_abs_max": float(dict(m.named_parameters())["transformer.mask_token"].abs().max())}))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
