"""CPU: whole-word masking in ``masking_collator`` (HF DataCollatorForWholeWordMask's rule per sentence) on toy-vocabulary sentences with
multi-piece words, and the unchanged draw of ``whole_word_masking=False``."""
import pytest
import torch

import rmcl_pkg  # noqa: F401
from rmcl_amd.attack.word_substitution import load_tokenizer
from rmcl_amd.vilt.datamodules.datamodule_base import continuation_ids_of
from rmcl_amd.vilt.datasets.base_dataset import masking_collator
from tests.datamodule_toy import VOCAB, caption

SPECIAL = (100, 101, 102, 103)        # [UNK] [CLS] [SEP] [MASK] of the toy vocabulary; [PAD] = 0
MASK, V, LEN = 103, 1148, 16


@pytest.fixture(scope="module")
def tok():
    return load_tokenizer(VOCAB)


def _words(tok, ids):
    """word = a piece and its ## followers; special / pad tokens belong to no word"""
    words = []
    open_word = False
    for t, p in enumerate(tok.convert_ids_to_tokens(ids)):
        if ids[t] in SPECIAL or ids[t] == 0:
            open_word = False
            continue
        if open_word and p.startswith("##"):
            words[-1].append(t)
        else:
            words.append([t])
        open_word = True
    return words


@pytest.mark.parametrize("prob", [0.15, 0.4])
def test_whole_words_budget_and_shares(tok, prob):
    sentences = [caption(k) for k in range(400)] + ["two dogs", "dogs", "walking houses kids jumped"]
    encs = [tok(s, truncation=True, max_length=LEN, padding="max_length") for s in sentences]
    assert any(sum(p.startswith("##") for p in tok.convert_ids_to_tokens(e["input_ids"])) >= 2 for e in encs)
    col = masking_collator(MASK, V, special_ids=SPECIAL, mlm_prob=prob, max_text_len=LEN, generator=torch.Generator().manual_seed(5),
                           whole_word_masking=True, continuation_ids=continuation_ids_of(tok))
    n_mask = n_keep = n_total = 0
    multi = 0
    for rep in range(6):
        out = col(encs)
        for e, ids, lab in zip(encs, out["input_ids"].tolist(), out["labels"].tolist()):
            plain = e["input_ids"]
            chosen = {t for t, v in enumerate(lab) if v != -100}
            assert all(lab[t] == plain[t] for t in chosen) and all(ids[t] == plain[t] for t in range(LEN) if t not in chosen)
            assert not any(plain[t] in SPECIAL or plain[t] == 0 for t in chosen)            # no special, no pad token
            words = _words(tok, plain)
            picked = [w for w in words if set(w) <= chosen]
            assert chosen == {t for w in picked for t in w}                                    # a union of whole words
            n_tokens = sum(1 for v in plain if v != 0)
            budget = min(512, max(1, int(round(n_tokens * prob))))
            n = len(chosen)
            assert n <= budget
            for w in words:
                if not set(w) <= chosen:
                    assert n + len(w) > budget, (plain, sorted(chosen), w, budget)             # every word left out would not have fitted
            multi += sum(len(w) > 1 for w in picked)
            n_total += n
            n_mask += sum(ids[t] == MASK for t in chosen)
            n_keep += sum(ids[t] == plain[t] for t in chosen)
    assert n_total >= 2000 and multi > 50
    # 80 / 10 / 10 within 5 sigma of the binomial.  A random replacement hits the original id or [MASK] with probability 1 / V each:
    # below a thousandth of the 10 % share, far inside the band
    band = lambda k, p: abs(k - n_total * p) <= 5 * (n_total * p * (1 - p)) ** 0.5
    assert band(n_mask, 0.8) and band(n_keep, 0.1) and band(n_total - n_mask - n_keep, 0.1), (n_mask, n_keep, n_total)


def test_word_order_is_random_and_seeded(tok):
    encs = [tok(caption(k), truncation=True, max_length=LEN, padding="max_length") for k in range(40)]
    make = lambda seed: masking_collator(MASK, V, special_ids=SPECIAL, mlm_prob=0.15, max_text_len=LEN, generator=torch.Generator().manual_seed(seed),
                                         whole_word_masking=True, continuation_ids=continuation_ids_of(tok))(encs)
    a, b, c = make(1), make(1), make(2)
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["input_ids"], b["input_ids"]) and not torch.equal(a["labels"], c["labels"])
    first_word = sum(int(l[1] != -100) for l in a["labels"].tolist())
    assert 0 < first_word < 40                                            # not always the first word, not never


def test_token_masking_draws_what_it_drew_before(tok):
    """whole_word_masking=False: the tensors of the commit before whole-word masking existed, recorded from a run of that commit with this
    seed on these sentences"""
    S = ["two dogs walking near the houses", "a child played in the home", "the lady jumped over a table", "three kids running from the red boat"]
    encs = [tok(s, truncation=True, max_length=12, padding="max_length") for s in S]
    for kw in ({}, {"continuation_ids": continuation_ids_of(tok)}):
        out = masking_collator(103, 1148, special_ids=(100, 101, 102, 103), mlm_prob=0.3, max_text_len=12, generator=torch.Generator().manual_seed(17),
                               **kw)(encs)
        assert out["input_ids"].tolist() == [[101, 1017, 1023, 1143, 103, 1144, 1011, 1002, 1048, 103, 102, 0],
                                             [101, 103, 1043, 103, 103, 103, 1002, 1049, 102, 0, 0, 0],
                                             [101, 1002, 1039, 103, 1145, 1016, 103, 1078, 102, 0, 0, 0],
                                             [101, 1018, 1044, 570, 100, 103, 1002, 1093, 1063, 102, 0, 0]]
        assert out["labels"].tolist() == [[-100, -100, -100, 1143, 1108, -100, -100, -100, -100, 1143, -100, -100],
                                          [-100, 1000, -100, 1138, 1145, 1004, -100, -100, -100, -100, -100, -100],
                                          [-100, -100, -100, 1123, 1145, -100, 1000, -100, -100, -100, -100, -100],
                                          [-100, -100, -100, 1143, -100, 1014, -100, -100, -100, -100, -100, -100]]


def test_whole_words_need_the_continuation_ids():
    with pytest.raises(NotImplementedError, match="continuation_ids"):
        masking_collator(MASK, V, whole_word_masking=True)
