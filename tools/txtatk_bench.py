"""Text view of the attacked VQA / NLVR2 fine-tuning steps on the MI355X: JSON lines in bench.py's style, appended to
profiles/txtatk_bench.jsonl.

  python tools/txtatk_bench.py --task vqa --bs 128 [--layers 12] [--dtype bf16] [--max-loops 10] [--n-candidates 5] [--steps 3] [--warmup 1]
  python tools/txtatk_bench.py --task nlvr2 --bs 64

Per task, with the toy linguistic files of tests/golden (vocabulary, counter-fitted vectors, stop words):
* ms per optimizer step (training_step + backward + fused AdamW) of the image-only step (the parent commit's step), the text-only step
  and the step with both views - host clock around steps that end in a device synchronise;
* the text attack of one step split into encoder passes / pooler passes / task head + loss + read-back + selection (what is left of
  get_grad and score) / host linguistic work (tokenising candidates; choosing words and building sentences) / word scoring, from a run of its own in which every timed section ends in a synchronise (the sections then
  do not overlap, so their sum exceeds the attack's share of the free-running step);
* word scoring, device against host, on the SAME saliency gradient in one process, alternating: Engine.word_saliency + the [B, W]
  read-back against the [B, L, D] copy + WS.importance_scores (medians of 20 each)."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_pkg  # noqa: F401,E402
from rmcl_amd.attack import greedy_attack_vilt as GA  # noqa: E402
from rmcl_amd.attack import word_substitution as WS  # noqa: E402
from rmcl_amd.vilt.config import task_finetune_vqa_randaug_attacked, task_finetune_nlvr2_randaug_attacked  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS, vilt_utils  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SENTENCES = [
    "a big dog and a small cat run on the green field near the house",
    "the man and the woman walk on the street with a child holding a red ball",
    "two dogs jump over a table in the house",
    "a lady is sitting in a boat looking at the kid playing with some puppy near a car",
    "the kitten eat under the desk",
    "three men hold the large football on a lawn by the road and look at the ship",
]


def batch_of(task, B, cfg, dev, tok, seed=0):
    g = torch.Generator().manual_seed(seed)
    text = [SENTENCES[b % len(SENTENCES)] for b in range(B)]
    ids, masks = WS.encode_sentences(tok, text, cfg["max_text_len"])
    S = cfg["image_size"]
    img = lambda: (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    out = {"text": text, "text_ids": ids.to(dev), "text_masks": masks.to(dev)}
    if task == "vqa":
        labels = [torch.randint(0, cfg["vqav2_label_size"], (int(torch.randint(0, 11, (1,), generator=g)),), generator=g).tolist() for _ in range(B)]
        out.update(image=[img()], vqa_labels=labels, vqa_scores=[torch.rand(len(l), generator=g).tolist() for l in labels], qid=list(range(B)))
    else:
        out.update(image_0=[img()], image_1=[img()], answers=[bool(x) for x in torch.randint(0, 2, (B,), generator=g).tolist()],
                   table_name=["nlvr2_train"] * B)
    return out


def module_of(task, a, text_view, image_view):
    kw = dict(num_layers=a.layers, per_gpu_batchsize=a.bs, adv_steps_img=a.adv_steps, max_steps=10 ** 6, warmup_steps=0, dense_images=True,
              text_view=text_view, image_view=image_view, max_loops=a.max_loops, n_candidates=a.n_candidates,
              tokenizer=os.path.join(GOLD, "toy_vocab.txt"), embedding_path=os.path.join(GOLD, "toy_counter_fitted.txt"),
              stopwords=os.path.join(GOLD, "toy_stopwords.txt"))
    cfg = task_finetune_vqa_randaug_attacked(**kw) if task == "vqa" else task_finetune_nlvr2_randaug_attacked(**kw)
    m = ViLTransformerSS(cfg, device="cuda:0", compute_dtype=a.dtype)
    vilt_utils.set_task(m)
    m.train()
    return m, cfg


def step_ms(m, batch, steps, warmup):
    (opt,), _ = m.configure_optimizers()
    loss = None
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        m.zero_grad()
        loss = m.training_step(batch, i)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / max(1, steps), float(loss)


class Sections:
    """wall time of wrapped callables, each ending in a device synchronise; nested sections are subtracted from their parent"""

    def __init__(self):
        self.ms, self.stack = {}, []

    def wrap(self, obj, name, section):
        fn = getattr(obj, name)

        def timed(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.stack.append(0.0)
            try:
                return fn(*args, **kw)
            finally:
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                inner = self.stack.pop()
                self.ms[section] = self.ms.get(section, 0.0) + dt - inner
                if self.stack:
                    self.stack[-1] += dt

        setattr(obj, name, timed)


def attack_split(m, batch):
    """one text attack with synchronised sections: {section: ms}"""
    att, eng = m.greedy_attacker, m.engine
    sec = Sections()
    sec.wrap(att, "adv_attack_samples", "other_host")
    # what is left of get_grad / score once the encoder and pooler passes are taken out: the task head, its loss, the gather of the
    # owners' labels, the candidate-row read-back and the host-side selection
    sec.wrap(att, "get_grad", "task_head_loss_readback_select")
    sec.wrap(att, "score", "task_head_loss_readback_select")
    sec.wrap(eng, "encoder_forward", "encoder_passes")
    sec.wrap(eng, "encoder_backward", "encoder_passes")
    sec.wrap(eng, "heads_forward", "pooler_passes")
    sec.wrap(eng, "heads_backward", "pooler_passes")
    sec.wrap(att, "get_inputs", "host_tokenising")
    sec.wrap(att, "word_scores", "word_scoring")
    sec.wrap(att, "compute_word_importance", "host_word_choice")
    sec.wrap(att, "construct_new_samples", "host_word_choice")
    sec.wrap(att, "calc_words_to_sub_words", "host_tokenising")
    att.adv_attack_samples(m, batch, None)
    for obj, names in ((att, ("adv_attack_samples", "get_grad", "score", "get_inputs", "word_scores", "compute_word_importance",
                              "construct_new_samples", "calc_words_to_sub_words")), (eng, ("encoder_forward", "encoder_backward", "heads_forward", "heads_backward"))):
        for n in names:
            delattr(obj, n)                                  # back to the class's methods
    return {k: round(v, 3) for k, v in sec.ms.items()}


def word_scoring_ab(m, batch, reps=20):
    """device against host on the same gradient, alternating: (device ms, host ms, max relative difference of the scores)"""
    att, eng = m.greedy_attacker, m.engine
    dev = eng.device
    tok = att.tokenizer
    ids, masks = batch["text_ids"].cpu(), batch["text_masks"].cpu()
    Bn, Lt = ids.shape
    words = [WS.decode_words(tok, ids[b]) for b in range(Bn)]
    att.calc_words_to_sub_words(words, Bn)
    pb, op = att.bind_batch(m, batch, ids.to(dev), masks.to(dev))
    de = torch.empty(att.saliency_rows(pb) * Lt, eng.cfg["hidden_size"], device=dev)
    att.set_text(pb, ids.to(dev), masks.to(dev))
    _, grads, _ = att.get_grad(m, pb, op, de)
    t_dev, t_host = [], []
    for i in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = att.word_scores(m, pb, grads, Bn)
        t1 = time.perf_counter()
        g = grads.cpu().numpy()
        b = [WS.importance_scores(g[s][1:], att.words_to_sub_words[s]) for s in range(Bn)]
        t2 = time.perf_counter()
        if i >= 3:
            t_dev.append((t1 - t0) * 1e3)
            t_host.append((t2 - t1) * 1e3)
    diff = max(float(np.max(np.abs(np.array(x) - np.array(y)) / np.abs(np.array(y)))) for x, y in zip(a, b) if len(y))
    return float(np.median(t_dev)), float(np.median(t_host)), diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=["vqa", "nlvr2"], default="vqa")
    ap.add_argument("--bs", type=int, default=None, help="samples (VQA, default 128) / pairs (NLVR2, default 64)")
    ap.add_argument("--adv-steps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--max-loops", type=int, default=10)
    ap.add_argument("--n-candidates", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txtatk_bench.jsonl"))
    a = ap.parse_args()
    a.bs = a.bs or (128 if a.task == "vqa" else 64)
    if not torch.cuda.is_available():
        sys.exit("txtatk_bench: no GPU - nothing is measured on the CPU")
    base = {"metric": "txtatk_step_ms", "task": f"{a.task}_attacked", "bs": a.bs, "layers": a.layers, "dtype": a.dtype, "adv_steps": a.adv_steps,
            "max_loops": a.max_loops, "n_candidates": a.n_candidates}
    lines = []
    for views, (tv, iv) in (("image", (False, True)), ("text", (True, False)), ("both", (True, True))):
        m, cfg = module_of(a.task, a, tv, iv)
        batch = batch_of(a.task, a.bs, cfg, "cuda:0", WS.load_tokenizer(os.path.join(GOLD, "toy_vocab.txt")))
        ms, loss = step_ms(m, batch, a.steps, a.warmup)
        line = dict(base, views=views, ms_per_step=round(ms, 2), loss=loss)
        if views == "text":
            line["attack_split_ms"] = attack_split(m, batch)
            d, h, diff = word_scoring_ab(m, batch)
            line.update(word_scoring_device_ms=round(d, 3), word_scoring_host_ms=round(h, 3), word_scoring_max_rel_diff=diff,
                        num_changes=float(m.logged[f"{a.task}_attacked_attack/train/num_changes"]))
        lines.append(line)
        print(json.dumps(line), flush=True)
        del m, batch
        gc.collect()                              # the module's deferred-backward closures form cycles: collect before the next one is built
        torch.cuda.empty_cache()
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
