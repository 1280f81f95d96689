"""Rehearsal of the guarded optimizer step with N > 1 on ONE GPU (developer / test use, never a measurement): every rank of a
torch.distributed.run launch sits on cuda:0, gloo replaces RCCL (which refuses two ranks on one device).  task_moco, 2 layers, bf16, PGD
K = 1, config skip_nonfinite_steps.  Three optimizer steps on another batch per rank:

  1. clean;
  2. two accumulated micro-steps; after the FIRST (sync_grads = False: no reduction) the last rank writes inf into one element of its
     LOCAL gradient arena, the second micro-step's reduction then carries it to every rank;
  3. clean.

No rank tells another what it decided: each runs the statistics pass on the reduced gradient it holds.  Prints one JSON line (rank 0):
the (applied, skipped) counters of every rank, whether step 2 left every rank's parameters, moments and bf16 shadow untouched, and whether
the parameter arenas of all ranks hold the same bits after step 3.

  python -m torch.distributed.run --nproc-per-node 2 tools/guarded_two_rank.py"""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch_of(cfg, B, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    S, Lt = cfg["image_size"], cfg["max_text_len"]
    ids = torch.randint(1000, cfg["vocab_size"], (B, Lt), generator=g, dtype=torch.int64)
    ids[:, 0], ids[:, -1] = 101, 102
    return {"image": [(torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(device)], "text": ["synthetic"] * B, "text_ids": ids.to(device),
            "text_masks": torch.ones(B, Lt, dtype=torch.int64, device=device), "text_labels": torch.full((B, Lt), -100, dtype=torch.int64, device=device)}


def fingerprint(*tensors):
    """Three exact integer sums over the bits of every tensor (int64: no rounding, no dependence on the summation order)."""
    out = []
    for t in tensors:
        v = t.detach().contiguous().view(torch.int32).long()
        out += [v.sum(), v[::7].sum(), v.abs().sum()]
    return torch.stack(out).cpu()


def main():
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.vilt.config import task_moco
    from rmcl_amd.vilt.modules import ViLTransformerSS
    torch.manual_seed(0)                                                  # the same initial weights and queue on every rank
    B = 4
    cfg = task_moco(num_layers=2, num_negative=1024, per_gpu_batchsize=B, adv_steps_img=1, vocab_size=2048, drop_rate=0.1, image_view=True,
                    num_gpus=world, num_nodes=1, max_steps=100, warmup_steps=0, learning_rate=1e-4, skip_nonfinite_steps=True)
    m = ViLTransformerSS(cfg, device="cuda:0", compute_dtype="bf16")
    (opt,), _ = m.configure_optimizers()
    m.train()
    e = m.engine
    batches = [batch_of(cfg, B, 100 + 10 * rank + i, "cuda:0") for i in range(4)]

    def micro(i, sync):
        m.sync_grads = sync
        m.training_step(batches[i], i).backward()

    micro(0, True)                                                        # step 1
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    before = fingerprint(e.q32, opt.m, opt.v, e.q_lp)
    micro(1, False)                                                       # step 2: poisoned on the last rank before the reduction
    if rank == world - 1:
        e.g32[4321] = float("inf")
    micro(2, True)
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    untouched = bool(torch.equal(fingerprint(e.q32, opt.m, opt.v, e.q_lp), before))
    after_skip = opt.counters()
    micro(3, True)                                                        # step 3
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    moved = not torch.equal(fingerprint(e.q32), before[:3])
    mine = torch.cat([fingerprint(e.q32, opt.m, opt.v), torch.tensor([*after_skip, *opt.counters(), int(untouched), int(moved)], dtype=torch.int64)])
    every = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    if rank == 0:
        print(json.dumps({"world_size": world,
                          "counters_after_skip": [[int(x[9]), int(x[10])] for x in every],
                          "counters_final": [[int(x[11]), int(x[12])] for x in every],
                          "skipped_step_wrote_nothing": [bool(x[13]) for x in every],
                          "clean_step_moved_the_weights": [bool(x[14]) for x in every],
                          "ranks_bit_identical": all(torch.equal(x[:9], every[0][:9]) for x in every),
                          "finite": bool(torch.isfinite(e.q32).all())}))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
