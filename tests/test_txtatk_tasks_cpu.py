"""CPU: the text view of the attacked VQA / NLVR2 tasks without a GPU - the CPU oracle (tests/txtatk_tasks_oracle.py) reproduces every
decision and loss the reference recorded in tests/golden/txtatk_{vqa,nlvr2}_L2_B4.npz, the fixtures meet their margin condition, the
argument checks of rmcl_word_saliency (its ctypes layout), the selection rule and span packing of the product against the oracle's, and
the new kernel's gfx950 assembly (present, no scratch)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import rmcl_pkg  # noqa: F401
from rmcl_amd import _lib as L
from rmcl_amd.attack import greedy_attack_vilt as GA
from tests import txtatk_tasks_oracle as T
from tests.golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REPLAY = {}


def _case(task):
    """fixture and its replay by the oracle, computed once per task and shared by the tests below"""
    if task not in _REPLAY:
        g = load(T.FIXTURE[task])
        _REPLAY[task] = (g, T.replay(task, g))
    return _REPLAY[task]


@pytest.mark.parametrize("task", ["vqa", "nlvr2"])
def test_oracle_reproduces_every_recorded_decision_and_loss(task):
    g, rp = _case(task)
    loops = int(g["meta"][6])
    assert rp["replace_idx"] == g["replace_idx"].tolist()                      # the word attacked, per loop and sample (-1: none eligible)
    assert rp["picks"] == g["best_idx"].tolist()                               # the candidate picked
    assert rp["changes_verification"] == g["changes_verification"].tolist()
    for li in range(loops):
        # candidate losses: fp32 reference against the oracle's double-precision sum of fp32 rows - a few ulps of the loss
        np.testing.assert_allclose(rp["losses"][li], g[f"cand_loss_{li}"], rtol=2e-6)
    # decisions are safe on THIS machine too: what the oracle differs by stays far below every margin
    assert rp["loss_diff"] * 10 <= float(g["cand_margin"].min())
    assert rp["score_rel_diff"] * 10 <= float(g["word_gap"].min())


@pytest.mark.parametrize("task", ["vqa", "nlvr2"])
def test_fixture_meets_the_margin_condition(task):
    g, rp = _case(task)
    np.testing.assert_allclose(rp["cand_margin"], g["cand_margin"], rtol=0, atol=0)      # (recomputed from the recorded reference values)
    np.testing.assert_allclose(rp["word_gap"], g["word_gap"], rtol=1e-12)
    assert float(g["cand_margin"].min()) >= T.MARGIN_FACTOR * float(g["oracle_loss_diff"]) > 0
    assert float(g["word_gap"].min()) >= T.MARGIN_FACTOR * float(g["oracle_score_rel_diff"]) > 0
    assert int((g["changes_verification"] > 0).sum()) >= 2                               # at least two samples change a word
    assert bool((g["replace_idx"] == -1).any())                                          # a sample without an eligible word
    assert bool(((g["best_idx"] == 0) & (g["replace_idx"] >= 0)).any())                  # an accepted pick with index 0
    assert [str(t) for t in g["text_out"]] != [str(t) for t in g["text_in"]]


def test_nlvr2_saliency_is_the_embedding_gradient_of_the_image_1_pass():
    """word_embeddings is called twice per get_grad (infer1, infer2) and only emb_grads[0] is read (:894): the recorded gradient is the
    oracle's gradient of the SECOND call (image_1, token type 2) - autograd runs the later-built branch first - not the first call's and
    not the sum."""
    g, rp = _case("nlvr2")
    scale = float(g["grads_absmax"])
    d0, d1 = [float(x) for x in g["emb_grad_pass_diff"]]
    assert d1 < 1e-5 * scale and d0 > 0.1 * scale
    sub = int(768 // g["grads_loop0_sub"].shape[2])
    p0, p1 = rp["grads_loop0"][0][:, :, ::sub], rp["grads_loop0"][1][:, :, ::sub]
    rec = g["grads_loop0_sub"]
    assert float(np.abs(rec - p1).max()) < 1e-5 * scale
    assert float(np.abs(rec - p0).max()) > 0.1 * scale and float(np.abs(rec - (p0 + p1)).max()) > 0.1 * scale
    np.testing.assert_allclose(p0, g["oracle_grads_pass0_sub"], atol=1e-5 * scale)
    np.testing.assert_allclose(p1, g["oracle_grads_pass1_sub"], atol=1e-5 * scale)


def test_product_selection_and_spans_follow_the_oracle():
    rng = np.random.RandomState(4)
    for _ in range(20):
        B = int(rng.randint(1, 6))
        all_num = [int(rng.randint(1, 6)) for _ in range(B)]
        owner = [b for b in range(B) for _ in range(all_num[b])]
        s, c = rng.rand(B).tolist(), (rng.rand(len(owner)) * (0.0 if _ == 0 else 1.0)).tolist()
        pad = [0] * int(rng.randint(0, 4))                                               # the padded tail of the candidate batch is ignored
        got = GA._TaskAttack.select(s, c + [9.0] * len(pad), owner + pad, len(owner), B)
        ref = T.select(s, c, all_num, B)
        assert [j for _, j in got] == [j for _, j in ref]
        np.testing.assert_allclose([x for ls, _ in got for x in ls], [x for ls, _ in ref for x in ls], rtol=1e-15)
    # start at -1: a single candidate, or all candidates equal, picks index 0; acceptance needs a loss > 0
    att = GA._TaskAttack.__new__(GA._TaskAttack)
    assert GA._TaskAttack.select([0.5], [0.5], [0], 1, 1)[0][1] == 0
    assert att.accept([0.25, 0.1], 0) and not att.accept([0.0], 0) and not att.accept([0.3], -1)
    assert not GA.GreedyAttack.accept(att, [0.25, 0.1], 0) and GA.GreedyAttack.accept(att, [0.1, 0.25], 1)     # MoCo's rule: index > 0
    sp = GA.word_spans([{0: np.arange(0, 1), 1: np.arange(1, 4)}, {}], 3)
    assert sp.dtype == torch.int32 and sp.tolist() == [[[1, 1], [2, 3], [0, 0]], [[0, 0], [0, 0], [0, 0]]]


def test_word_level_only_and_local_resources():
    cfg = dict(max_text_len=40, n_candidates=5, max_loops=3, max_image_len=200, vocab_size=30522, tokenizer="bert-base-uncased",
               embedding_path="../attack/counter-fitted-vectors.txt")
    for cls in (GA.GreedyAttack_vqa, GA.GreedyAttack_nlvr2):
        with pytest.raises(NotImplementedError, match="local vocabulary"):
            cls(cfg)
        att = cls(dict(cfg, tokenizer=os.path.join(T.GOLD, "toy_vocab.txt"), embedding_path=os.path.join(T.GOLD, "toy_counter_fitted.txt"),
                       stopwords=os.path.join(T.GOLD, "toy_stopwords.txt")))
        assert att.tokenizer is not None and "dog" in att.synonyms


def test_word_saliency_checks_its_arguments_before_any_launch():
    """ctypes layout of rmcl_word_saliency(g, spans, out, B, W, L, D, row0, row_step, stream): each bad value is named by the check that
    sits at ITS position, on host buffers, without a GPU."""
    lib = L.lib
    f, i = (C.c_float * 64)(), (C.c_int32 * 64)()

    def err(rc, needle):
        assert rc == -1
        assert needle in lib.rmcl_last_error().decode()

    err(lib.rmcl_word_saliency(None, i, f, 1, 1, 8, 16, 0, 1, None), "word_saliency: NULL")
    err(lib.rmcl_word_saliency(f, None, f, 1, 1, 8, 16, 0, 1, None), "word_saliency: NULL")
    err(lib.rmcl_word_saliency(f, i, None, 1, 1, 8, 16, 0, 1, None), "word_saliency: NULL")
    for bad in ((0, 1, 8, 16, 0, 1), (1, 0, 8, 16, 0, 1), (1, 1, 0, 16, 0, 1), (1, 1, 8, 18, 0, 1), (1, 1, 8, 0, 0, 1), (1, 1, 8, 16, -1, 1),
                (1, 1, 8, 16, 0, 0), (1, 4097, 8, 16, 0, 1), (1, 1, 4097, 16, 0, 1), (1, 1, 8, 8196, 0, 1), (65537, 1, 8, 16, 0, 1)):
        err(lib.rmcl_word_saliency(f, i, f, *bad, None), "word_saliency: bad shape")
    assert "rmcl_word_saliency" in L.EXPORTS


@pytest.fixture(scope="module")
def isa():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    src = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc", "txtatk.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only",
             "-I" + os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "txtatk.s")
        r = subprocess.run(["hipcc", *flags, src, "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(dst).read()


def test_txtatk_kernels_are_present_and_use_no_scratch(isa):
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    assert "word_saliency_kernel" in " ".join(n for n, _ in sizes)
    spilled = [(n[:80], int(s)) for n, s in sizes if int(s) != 0]
    assert not spilled, spilled
    body = isa.split("word_saliency_kernel", 1)[1]
    assert "global_load_dwordx4" in body                                     # the gradient rows are read as float4
