"""NLVR2 fine-tuning step on the MI355X: one JSON line per configuration, in bench.py's style.

  python tools/nlvr2_bench.py [--pairs 64 128] [--adv-steps 5] [--steps 20] [--warmup 5] [--layers 12] [--dtype bf16] [--forms pair two]
                              [--tasks clean attacked]

For every (task, pairs, form): ms per optimizer step (training_step + backward + fused AdamW; clean: task_finetune_nlvr2, attacked:
task_finetune_nlvr2_randaug_attacked with the image view, attack_idx [True, True]) and pairs/s; form "pair" runs both images of a pair
as ONE encoder pass of 2B sequences (nlvr2_pair_pass, the default), "two" the reference's two passes.  Then the head + CE alone, forward
(head forward + CE) and backward (CE gradient + head backward with weight gradients), each timed with events in isolation."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_pkg  # noqa: F401,E402
from rmcl_amd.vilt.config import task_finetune_nlvr2, task_finetune_nlvr2_randaug_attacked  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402


def batch_of(B, cfg, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = cfg["max_text_len"]
    ids = torch.randint(1000, cfg["vocab_size"], (B, L), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    S = cfg["image_size"]
    img0 = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    img1 = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    answers = [bool(x) for x in torch.randint(0, 2, (B,), generator=g).tolist()]
    return {"image_0": [img0.to(dev)], "image_1": [img1.to(dev)], "text_ids": ids.to(dev),
            "text_masks": torch.ones(B, L, dtype=torch.int64, device=dev), "text": ["x"] * B, "answers": answers,
            "table_name": ["nlvr2_dev"] * B}


def run(a, task, B, form, dev):
    kw = dict(num_layers=a.layers, per_gpu_batchsize=B, adv_steps_img=a.adv_steps, max_steps=10 ** 6, warmup_steps=0, dense_images=True,
              nlvr2_pair_pass=form == "pair")
    cfg = task_finetune_nlvr2(**kw) if task == "clean" else task_finetune_nlvr2_randaug_attacked(image_view=True, **kw)
    m = ViLTransformerSS(cfg, device=dev, compute_dtype=a.dtype)
    (opt,), _ = m.configure_optimizers()
    m.train()
    batch = batch_of(B, cfg, dev)
    loss = None
    for i in range(a.warmup + a.steps):
        if i == a.warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        m.zero_grad()
        loss = m.training_step(batch, i)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / max(1, a.steps)
    eng = m.engine
    nb = eng.nlvr2_bufs(B, "nlvr2" if task == "clean" else "att")
    cls2 = torch.randn(B, 2 * cfg["hidden_size"], device=dev)
    one = torch.ones(1, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fw, bw = [], []
    for i in range(30):
        ev[0].record()
        eng.nlvr2_forward(nb, cls2)
        eng.nlvr2_ce(nb, 1.0, want_dz=False)
        ev[1].record()
        eng.nlvr2_ce(nb, 1.0, want_dz=True, scale_dev=one)
        eng.nlvr2_backward(nb, nb.dz, with_grads=True)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= 5:
            fw.append(ev[0].elapsed_time(ev[1]))
            bw.append(ev[1].elapsed_time(ev[2]))
    fw.sort()
    bw.sort()
    print(json.dumps({"metric": "nlvr2_finetune_step_ms", "task": "nlvr2" if task == "clean" else "nlvr2_attacked", "pairs": B,
                      "form": form, "adv_steps": 0 if task == "clean" else a.adv_steps, "layers": a.layers, "dtype": a.dtype,
                      "ms_per_step": round(ms, 3), "pairs_per_s": round(B / ms * 1e3, 1), "head_ce_fwd_ms": round(fw[len(fw) // 2], 4),
                      "head_ce_bwd_ms": round(bw[len(bw) // 2], 4), "loss": float(loss)}), flush=True)
    del m, opt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--adv-steps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--forms", nargs="+", default=["pair", "two"])
    ap.add_argument("--tasks", nargs="+", default=["clean", "attacked"])
    a = ap.parse_args()
    for task in a.tasks:
        for B in a.pairs:
            for form in a.forms:
                run(a, task, B, form, "cuda:0")


if __name__ == "__main__":
    main()
