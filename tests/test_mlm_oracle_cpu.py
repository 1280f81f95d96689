"""CPU: tests/mlm_oracle.py (the MLM head, loss and accuracy restated in torch) against every mlm_* fixture recorded from the
reference's own compute_mlm run, the row compaction restated in numpy, and the invariants of masking_collator (the BERT rule of the
reference's datamodule, pinned by its own statistics - not by HF's random stream)."""
import numpy as np
import pytest
import torch

import rmcl_pkg  # noqa: F401
from oracle import rmcl_oracle as O
from rmcl_amd.vilt.datasets.base_dataset import masking_collator, default_collator, collate
from tests import mlm_oracle as M
from tests.golden_util import digest

TOL = dict(loss=1e-3, logits=2e-3, grad=2e-3)        # the f32 tolerances of tests/test_mlm_gpu.py


@pytest.mark.parametrize("name", M.FIXTURES)
def test_oracle_matches_reference_golden(name):
    g, cfg, p, batch, with_itm = M.load_case(name)
    torch.set_num_threads(16)
    for n_, t in p.items():
        if not n_.startswith("k_"):
            t.requires_grad_(True)
    r = M.compute_mlm(p, cfg, batch)
    n = int(g["n"])
    assert r["n"] == n and r["correct"] == int(g["correct"])
    loss = r["mlm_loss"]
    if with_itm:
        ri = O.compute_itm_wpa(p, cfg, batch, torch.from_numpy(g["itm_labels"]))
        assert abs(float(ri["itm_loss"]) - float(g["itm_loss"])) < TOL["loss"] * float(g["itm_loss"])
        loss = loss + ri["itm_loss"] + ri["itm_wpa_loss"]
        assert abs(float(loss) - float(g["total_loss"])) < TOL["loss"] * float(g["total_loss"])
    if n == 0:
        assert np.isnan(float(g["mlm_loss"])) and np.isnan(float(r["mlm_loss"]))
        # F.cross_entropy(ignore_index=-100) over an all-ignored batch: NaN loss, all-zero gradient (recorded from the reference)
        for nm, d in zip(g["grad_names"], g["grad_digest"]):
            assert d[1] == 0, str(nm)
        return
    assert abs(float(r["mlm_loss"]) - float(g["mlm_loss"])) < TOL["loss"] * float(g["mlm_loss"])
    assert abs(r["correct"] / n - float(g["log_accuracy"])) < 1e-6
    zmax = max(1.0, float(g["zmax"]))
    np.testing.assert_allclose(r["row_loss"].detach().numpy(), g["row_loss"], atol=TOL["loss"] * np.abs(g["row_loss"]).max())
    rows = r["mlm_rows"].detach()
    np.testing.assert_allclose(rows[:, torch.from_numpy(g["sample_cols"])].numpy(), g["sample_logits"], atol=TOL["logits"] * zmax)
    assert np.array_equal(rows.argmax(dim=1).numpy(), g["argmax"])
    top2 = rows.topk(2, dim=1).values
    np.testing.assert_allclose((top2[:, 0] - top2[:, 1]).numpy(), g["gap"], atol=2 * TOL["logits"] * zmax)
    assert float(g["gap"].min()) >= 0.1 * zmax                      # no near-tie row in the reference (bf16 logits tolerance)
    assert np.array_equal(batch["text_labels_mlm"][batch["text_labels_mlm"] != -100].numpy(), g["labels"])
    loss.backward()
    for nm, d in zip(g["grad_names"], g["grad_digest"]):
        got = digest(p[str(nm)].grad)
        assert abs(got[1] - d[1]) <= TOL["grad"] * d[1] + 1e-7, (str(nm), got[:3], d[:3])
    cols = torch.from_numpy(g["sample_cols"])
    np.testing.assert_allclose(p["mlm_score.decoder.weight"].grad[cols[:16], :64].numpy(), g["grad_decoder_w"],
                               atol=TOL["grad"] * 2.5 * np.abs(g["grad_decoder_w"]).max())
    np.testing.assert_allclose(p["mlm_score.bias"].grad[cols].numpy(), g["grad_mlm_bias"], atol=TOL["grad"] * 2.5 * np.abs(g["grad_mlm_bias"]).max())
    wr = torch.from_numpy(g["word_rows"])
    np.testing.assert_allclose(p["text_embeddings.word_embeddings.weight"].grad[wr, :64].numpy(), g["grad_word"],
                               atol=TOL["grad"] * 2.5 * np.abs(g["grad_word"]).max())


def test_ragged_fixture_holds_the_edge_cases():
    g, cfg, p, batch, _ = M.load_case("mlm_L2_B4_ragged")
    lab, masks = batch["text_labels_mlm"], batch["text_masks"]
    lens = masks.sum(dim=1)
    assert len(set(lens.tolist())) > 1                                # ragged text lengths
    assert bool((lab[0] == -100).all())                               # one sample with no masked token
    assert int(lab[1, 0]) != -100                                     # a masked first token
    assert int(lab[2, int(lens[2]) - 1]) != -100                      # a masked last valid token
    assert int(lab[1, 3]) == int(lab[3, 2]) == M.dominant_tokens(cfg, int(g["meta"][2]))[0]      # one label in two rows
    assert bool((lab[masks == 0] == -100).all())
    assert int(g["correct"]) == 2                                     # ... which is the head's dominant token: a non-trivial accuracy
    e = M.load_case("mlm_L2_B2_empty")
    assert int(e[0]["n"]) == 0 and bool((e[3]["text_labels_mlm"] == -100).all())


def test_compaction_restated_in_numpy():
    g = torch.Generator().manual_seed(3)
    B, Lt, N = 5, 40, 185
    lab = torch.full((B, Lt), -100, dtype=torch.int64)
    on = torch.rand(B, Lt, generator=g) < 0.15
    lab[on] = torch.randint(0, 30522, (int(on.sum()),), generator=g)
    rows, labels, n = M.compact(lab, N)
    want = [(b * N + l, int(lab[b, l])) for b in range(B) for l in range(Lt) if int(lab[b, l]) != -100]
    assert n == len(want) and rows.tolist() == [r for r, _ in want] and labels.tolist() == [l for _, l in want]
    assert rows.tolist() == sorted(rows.tolist())
    assert M.compact(torch.full((2, Lt), -100, dtype=torch.int64), N)[2] == 0


def _encodings(n_seq, g):
    encs = []
    for i in range(n_seq):
        k = 40 if i % 4 else int(torch.randint(8, 40, (1,), generator=g))
        ids = torch.randint(1000, 30522, (k,), generator=g).tolist()
        ids[0], ids[-1] = 101, 102
        encs.append({"input_ids": ids, "attention_mask": [1] * k})
    return encs


def test_masking_collator_invariants():
    V, MASK = 30522, 103
    g = torch.Generator().manual_seed(11)
    encs = _encodings(5200, g)                                        # > 200 000 tokens
    plain = default_collator(40)(encs)["input_ids"]
    col = masking_collator(MASK, V, special_ids=(101, 102), mlm_prob=0.15, max_text_len=40, generator=torch.Generator().manual_seed(5))
    out = col(encs)
    ids, lab = out["input_ids"], out["labels"]
    assert ids.shape == lab.shape == plain.shape and ids.dtype == lab.dtype == torch.int64
    chosen = lab != -100
    assert torch.equal(lab[chosen], plain[chosen])                    # labels = the original id on chosen positions ...
    assert torch.equal(ids[~chosen], plain[~chosen])                  # ... -100 exactly on the unchosen ones, which are unchanged
    special = (plain == 101) | (plain == 102) | (plain == 0)
    assert not bool((chosen & special).any())                         # special / pad positions are never chosen
    free = int((~special).sum())
    assert free >= 200000 - 2 * 5200 - 5200 * 32 // 4
    band = lambda k, nn, pp: abs(k - nn * pp) <= 4 * (nn * pp * (1 - pp)) ** 0.5      # binomial 4 sigma
    n = int(chosen.sum())
    assert band(n, free, 0.15), (n, free)
    masked = int((ids[chosen] == MASK).sum())
    same = int((ids[chosen] == plain[chosen]).sum())
    swapped = n - masked - same
    assert band(masked, n, 0.8) and band(same, n, 0.1) and band(swapped, n, 0.1), (masked, same, swapped, n)
    assert bool(((ids >= 0) & (ids < V)).all())
    again = masking_collator(MASK, V, special_ids=(101, 102), mlm_prob=0.15, max_text_len=40, generator=torch.Generator().manual_seed(5))(encs)
    assert torch.equal(again["input_ids"], ids) and torch.equal(again["labels"], lab)
    other = masking_collator(MASK, V, special_ids=(101, 102), generator=torch.Generator().manual_seed(6))(encs)
    assert not torch.equal(other["labels"], lab)
    none = masking_collator(MASK, V, special_ids=(101, 102), mlm_prob=0.0)(encs)
    assert bool((none["labels"] == -100).all()) and torch.equal(none["input_ids"], plain)
    with pytest.raises(NotImplementedError):
        masking_collator(MASK, V, whole_word_masking=True)


def test_masking_collator_feeds_collate():
    g = torch.Generator().manual_seed(2)
    encs = _encodings(4, g)
    samples = [{"image": [torch.zeros(3, 64, 64)], "text": ("t", e)} for e in encs]
    col = masking_collator(103, 30522, special_ids=(101, 102), mlm_prob=0.5, generator=torch.Generator().manual_seed(1))
    batch = collate(samples, col)
    assert batch["text_ids_mlm"].shape == batch["text_labels_mlm"].shape == batch["text_ids"].shape == (4, 40)
    on = batch["text_labels_mlm"] != -100
    assert bool(on.any()) and torch.equal(batch["text_labels_mlm"][on], batch["text_ids"][on])
    assert bool((batch["text_labels"] == -100).all())
