"""What the epoch metrics cost per step.

Kernel   stream time (device events around ITERS calls, medians over ROUNDS rounds that alternate the arms in one process) of the
         rmcl_metrics_update launches of
             vqa            a VQA step at B = 128: one launch, SCALAR loss + ROWSUM over rows[:, 1]
             mlm_itm_mpp    an mlm + itm + mpp step at B = 64: three launches, as the three objectives flush them
                            (PAIR + gated SCALAR, PAIR + gated SCALAR, ARGMAX_MATCH + 2 SCALAR)
         next to a torch restatement of the same accumulation into a float64 table (``*_torch``: one small launch per term).
Step     a trainer-driven task_finetune_vqa step (two layers, the toy data root of tests/datamodule_toy.py, batch 4) with the epoch metrics
         on and off: wall time of training_step + backward + optimizer step between device synchronisations, the two models alternating.

  python tools/metrics_bench.py --out profiles/epoch_metrics_bench.json"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS, ROUNDS, WARMUP = 50, 20, 5
STEP_ITERS = 3


def kernel_arms():
    import torch
    import rmcl_pkg  # noqa: F401
    from rmcl_amd.vilt.gadgets.my_metrics import EpochMetrics
    dev = "cuda:0"
    torch.manual_seed(0)
    em = EpochMetrics(dev)
    names = ["vqa_score", "vqa_loss", "mlm_acc", "mlm_loss", "mpp_acc", "mpp_loss", "itm_acc", "itm_loss", "itm_wpa"]
    for n in names:
        em.register(n)
    rows = torch.rand(128, 2, device=dev)
    loss = torch.rand(1, device=dev)
    stats = torch.tensor([2.5, 40.0, 96.0], device=dev)
    logits = torch.randn(64, 2, device=dev)
    labels = torch.randint(0, 2, (64,), device=dev, dtype=torch.int32)
    tab = torch.zeros(len(names), 2, dtype=torch.float64, device=dev)

    def vqa():
        em.rowsum("vqa_score", rows[:, 1], 128, stride=2)
        em.scalar("vqa_loss", loss)
        em.flush()

    def vqa_torch():
        tab[0, 0] += rows[:, 1].sum()
        tab[0, 1] += 128
        tab[1, 0] += loss[0]
        tab[1, 1] += 1

    def pre():
        for t in ("mlm", "mpp"):
            em.pair(f"{t}_acc", stats[1:2], stats[2:3])
            em.scalar(f"{t}_loss", stats[0:1], gate=stats[2:3])
            em.flush()
        em.argmax_match("itm_acc", logits, labels)
        em.scalar("itm_loss", loss)
        em.scalar("itm_wpa", loss)
        em.flush()

    def pre_torch():
        for i in (2, 4):
            tab[i, 0] += stats[1]
            tab[i, 1] += stats[2]
            on = (stats[2] != 0).to(torch.float64)         # (the gate of the loss: a batch without a labelled row adds nothing)
            tab[i + 1, 0] += torch.where(on > 0, stats[0].double(), on)
            tab[i + 1, 1] += on
        tab[6, 0] += (logits.argmax(-1) == labels).sum()
        tab[6, 1] += 64
        for i in (7, 8):
            tab[i, 0] += loss[0]
            tab[i, 1] += 1

    return {"vqa": vqa, "vqa_torch": vqa_torch, "mlm_itm_mpp": pre, "mlm_itm_mpp_torch": pre_torch}


def bench_kernels():
    import torch
    arms = kernel_arms()

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / ITERS * 1e3

    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            us[k].append(window(fn))
    return {k: {"us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for k, v in us.items()}


def bench_step():
    import torch
    import rmcl_pkg  # noqa: F401
    from rmcl_amd import trainer as T
    from rmcl_amd.vilt import config as C
    from rmcl_amd.vilt.datamodules import MTDataModule
    from rmcl_amd.vilt.modules import ViLTransformerSS, vilt_utils
    from tests.datamodule_toy import toy_config, write_toy_root
    with tempfile.TemporaryDirectory() as d:
        root = write_toy_root(d, only=["vqav2"])
        cfg = toy_config(C.task_finetune_vqa, root, max_steps=1000)
        dm = MTDataModule(cfg)
        dm.setup("fit")
        random.seed(0)
        torch.manual_seed(0)
        batch = next(iter(dm.train_dataloader()))
    models = {}
    for arm in ("off", "on"):
        torch.manual_seed(0)
        m = ViLTransformerSS(dict(cfg), device="cuda:0", compute_dtype="bf16")
        m.train()
        if arm == "on":
            vilt_utils.set_metrics(m)
        (opt,), (sd,) = m.configure_optimizers()
        models[arm] = (m, opt, sd["scheduler"], T.to_device(batch, m.device))

    def window(arm):
        m, opt, sched, b = models[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEP_ITERS):
            m.training_step(b, i).backward()
            opt.step()
            sched.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEP_ITERS * 1e3

    for arm in models:
        window(arm)
    ms = {arm: [] for arm in models}
    for _ in range(ROUNDS):
        for arm in models:
            ms[arm].append(window(arm))
    out = {f"metrics_{k}": {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}
    out["added_ms_median"] = out["metrics_on"]["ms_median"] - out["metrics_off"]["ms_median"]
    out["what"] = "task_finetune_vqa, 2 layers, toy batch of 4: training_step + backward + optimizer step, wall time between synchronisations"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"what": "rmcl_metrics_update per step: stream time of the launches of a VQA step (B = 128) and of an mlm + itm + mpp step (B = 64), each "
                   "beside a torch restatement; and a trainer-driven VQA step with the epoch metrics on and off",
           "iters_per_window": ITERS, "rounds": ROUNDS, "single_run": True, "kernel_us": bench_kernels(), "vqa_step_ms": bench_step()}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
