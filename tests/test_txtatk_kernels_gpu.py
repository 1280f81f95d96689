"""-m gpu: the word-saliency kernel of the text attack on the fine-tuning tasks (include/rmcl.h rmcl_word_saliency, csrc/txtatk.hip)
against a float64 reference, its bit-reproducibility, and the candidate-scoring helper that sends more rows than the VQA head launcher
takes (256) through it in chunks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmcl_pkg  # noqa: F401,E402
from rmcl_amd import _lib as L  # noqa: E402
from rmcl_amd._lib import lib, check, P  # noqa: E402
from rmcl_amd.attack import greedy_attack_vilt as GA  # noqa: E402
from rmcl_amd.attack import word_substitution as WS  # noqa: E402
from rmcl_amd.runtime import stream_ptr  # noqa: E402
from rmcl_amd.vilt.config import task_finetune_vqa  # noqa: E402
from rmcl_amd.vilt.modules import ViLTransformerSS  # noqa: E402
from tests import vqa_oracle as V  # noqa: E402

DEV = "cuda:0"
# worst-case bound n 2^-24 of an fp32 sum of n = 768 + len terms (every term rounded once): 4.6e-5 at n = 771 - no correct kernel exceeds it
RTOL = 5e-5


def _reference(g, spans, row0, row_step):
    """out[b, w] = sum_d | (1 / len) * sum_t g[row0 + b * row_step, t, d] | in float64"""
    B, W, _ = spans.shape
    out = np.zeros((B, W))
    g64 = g.double().numpy()
    for b in range(B):
        for w in range(W):
            s, n = int(spans[b, w, 0]), int(spans[b, w, 1])
            if n > 0:
                out[b, w] = np.abs(g64[row0 + b * row_step, s:s + n].sum(axis=0) / n).sum()
    return out


def _run(g, spans, L_, row0=0, row_step=1):
    B, W, _ = spans.shape
    out = torch.full((B, W), float("nan"), device=DEV)
    check(lib.rmcl_word_saliency(P(g), P(spans), P(out), B, W, L_, g.shape[-1], row0, row_step, stream_ptr()), "word_saliency")
    torch.cuda.synchronize()
    return out


def _big_case():
    """R = 6 sequences of L = 40, D = 768; B = 3 sentences of W = 39 entries: spans of length 1 and 3, one that ends on the last token,
    zero-count padding entries"""
    gen = torch.Generator().manual_seed(17)
    g = torch.randn(6, 40, 768, generator=gen) * torch.rand(6, 40, 1, generator=gen)
    spans = torch.zeros(3, 39, 2, dtype=torch.int32)
    for b in range(3):
        t, w = 1, 0
        while t < 40 and w < 39 - 4 * b:                       # sentence b leaves 4 b padding entries
            n = 3 if (w + b) % 4 == 1 and t + 3 <= 40 else 1
            spans[b, w] = torch.tensor([t, n])
            t, w = t + n, w + 1
    spans[2, 5] = torch.tensor([37, 3])                        # ends on the last token (positions 37, 38, 39)
    assert int((spans[:, :, 1] == 0).sum()) > 0 and int((spans[:, :, 1] == 3).sum()) > 0
    assert any(int(s) + int(n) == 40 for s, n in spans.view(-1, 2).tolist() if n)
    return g, spans


def test_word_saliency_smallest_shape_matches_fp64():
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(1, 8, 16, generator=gen)
    spans = torch.tensor([[[2, 3]]], dtype=torch.int32)
    out = _run(g.to(DEV), spans.to(DEV), 8)
    np.testing.assert_allclose(out.cpu().numpy(), _reference(g, spans, 0, 1), rtol=RTOL)


@pytest.mark.parametrize("row0,row_step", [(0, 1), (1, 2)])
def test_word_saliency_matches_fp64_and_is_bit_reproducible(row0, row_step):
    g, spans = _big_case()
    gd, sd = g.to(DEV), spans.to(DEV)
    out = _run(gd, sd, 40, row0, row_step)
    ref = _reference(g, spans, row0, row_step)
    got = out.cpu().numpy()
    pad = spans[:, :, 1].numpy() == 0
    assert np.all(got[pad] == 0.0) and not np.isnan(got).any()              # padding entries write exactly 0, every entry is written
    np.testing.assert_allclose(got[~pad], ref[~pad], rtol=RTOL)
    assert torch.equal(out, _run(gd, sd, 40, row0, row_step))               # one owner per output, fixed order: identical bits
    if row_step == 2:                                                       # the odd sequences, not the even ones
        assert not np.allclose(got[~pad], _reference(g, spans, 0, 2)[~pad], rtol=1e-3)


def test_engine_word_saliency_equals_the_host_path():
    """Engine.word_saliency on spans built from word <-> sub-word maps against WS.importance_scores on the copied gradient."""
    g, _ = _big_case()
    maps = [{0: np.arange(0, 1), 1: np.arange(1, 4), 2: np.arange(4, 5)}, {0: np.arange(0, 2)}, {i: np.arange(i, i + 1) for i in range(39)}]
    spans = GA.word_spans(maps, 39)
    m = ViLTransformerSS(task_finetune_vqa(num_layers=1, per_gpu_batchsize=2, drop_rate=0.0), device=DEV, compute_dtype="f32")
    out = m.engine.word_saliency(g.to(DEV).view(-1, 768), spans.to(DEV), 40, 1, 2).cpu().numpy()
    for b, mp in enumerate(maps):
        host = WS.importance_scores(g[1 + 2 * b].numpy()[1:], mp)
        np.testing.assert_allclose(out[b, :len(mp)], host, rtol=RTOL)
        assert np.all(out[b, len(mp):] == 0.0)
    with pytest.raises(L.RmclError):
        m.engine.word_saliency(g.to(DEV), spans.to(DEV), 40, 2, 2)          # sentence 2 would read sequence 6 of 6


def test_candidate_rows_go_through_the_vqa_head_in_chunks():
    """257 candidate rows (the launcher takes 256): per-row BCE sums against the unchunked torch arithmetic in fp64."""
    R, A = 257, 3
    m = ViLTransformerSS(task_finetune_vqa(num_layers=1, per_gpu_batchsize=2, drop_rate=0.0), device=DEV, compute_dtype="f32")
    eng = m.engine
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, prm in m.named_parameters():
            if n.startswith("vqa_classifier.") and n.endswith("bias"):
                prm.copy_(0.3 * torch.randn(prm.shape, generator=gen).to(DEV))
    cls = torch.randn(R, 768, generator=gen)
    labels = torch.randint(0, V.N_LABELS, (R, A), generator=gen).to(torch.int32)
    labels[::5, 2] = -1                                                      # pads
    labels[256] = torch.tensor([7, 7, 9])                                    # the row behind the chunk boundary: a repeated label
    scores = torch.rand(R, A, generator=gen)
    out = GA.vqa_candidate_rows(eng, cls.to(DEV), labels.to(DEV), scores.to(DEV), A)
    torch.cuda.synchronize()
    w = {n: prm.detach().cpu().double() for n, prm in m.named_parameters() if n.startswith("vqa_classifier.")}
    z = V.vqa_head(w, cls.double())
    tgt = V.dense_targets([[int(x) for x in r if x >= 0] for r in labels.tolist()],
                          [[float(s) for x, s in zip(r, sr) if x >= 0] for r, sr in zip(labels.tolist(), scores.tolist())], R, dtype=torch.float64)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(z, tgt, reduction="none").sum(1)
    assert torch.allclose(out.cpu().double(), ref, rtol=1e-5)                # (the per-row tolerance of tests/test_vqa_gpu.py)
