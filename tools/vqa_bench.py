"""VQAv2 fine-tuning step on the MI355X: one JSON line in bench.py's style.

  python tools/vqa_bench.py --bs 128 --adv-steps 5 --steps 20 --warmup 5 [--clean] [--layers 12] [--dtype bf16]

ms per optimizer step (training_step + backward + fused AdamW; --clean: the task_finetune_vqa step, otherwise
task_finetune_vqa_randaug_attacked with the image view) and pairs/s, the loss, and the head + BCE alone per pass, forward
(head forward + BCE) and backward (BCE gradient + head backward with weight gradients), each timed with events in isolation."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_pkg  # noqa: F401,E402
from rmcl_amd.vilt.config import task_finetune_vqa, task_finetune_vqa_randaug_attacked  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402


def batch_of(B, cfg, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = cfg["max_text_len"]
    ids = torch.randint(1000, cfg["vocab_size"], (B, L), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    img = torch.rand(B, 3, cfg["image_size"], cfg["image_size"], generator=g) * 2 - 1
    labels = [torch.randint(0, cfg["vqav2_label_size"], (int(torch.randint(0, 11, (1,), generator=g)),), generator=g).tolist() for _ in range(B)]
    scores = [torch.rand(len(l), generator=g).tolist() for l in labels]
    return {"image": [img.to(dev)], "text_ids": ids.to(dev), "text_masks": torch.ones(B, L, dtype=torch.int64, device=dev),
            "text": ["x"] * B, "vqa_labels": labels, "vqa_scores": scores, "qid": list(range(B))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--adv-steps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--clean", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    kw = dict(num_layers=a.layers, per_gpu_batchsize=a.bs, adv_steps_img=a.adv_steps, max_steps=10 ** 6, warmup_steps=0, dense_images=True)
    cfg = task_finetune_vqa(**kw) if a.clean else task_finetune_vqa_randaug_attacked(image_view=True, **kw)
    m = ViLTransformerSS(cfg, device=dev, compute_dtype=a.dtype)
    (opt,), _ = m.configure_optimizers()
    m.train()
    batch = batch_of(a.bs, cfg, dev)
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
    # head + BCE in isolation (the buffers of the last step's view)
    eng = m.engine
    vb = eng.vqa_bufs(a.bs, "vqa" if a.clean else "vqa_att")
    cls = torch.randn(a.bs, cfg["hidden_size"], device=dev)
    one = torch.ones(1, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fw, bw = [], []
    for i in range(30):
        ev[0].record()
        eng.vqa_forward(vb, cls)
        eng.vqa_bce(vb, 1.0, want_dz=False)
        ev[1].record()
        eng.vqa_bce(vb, 1.0, want_dz=True, scale_dev=one)
        eng.vqa_backward(vb, vb.dz, with_grads=True)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= 5:
            fw.append(ev[0].elapsed_time(ev[1]))
            bw.append(ev[1].elapsed_time(ev[2]))
    fw.sort()
    bw.sort()
    print(json.dumps({"metric": "vqa_finetune_step_ms", "task": "vqa" if a.clean else "vqa_attacked", "bs": a.bs,
                      "adv_steps": 0 if a.clean else a.adv_steps, "layers": a.layers, "dtype": a.dtype, "ms_per_step": round(ms, 3),
                      "pairs_per_s": round(a.bs / ms * 1e3, 1), "head_fwd_ms": round(fw[len(fw) // 2], 4),
                      "head_bwd_ms": round(bw[len(bw) // 2], 4), "loss": float(loss)}))


if __name__ == "__main__":
    main()
