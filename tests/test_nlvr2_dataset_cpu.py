"""CPU: NLVR2Dataset against the reference's own NLVR2Dataset on two tiny shards (tests/golden/nlvr2_dev.arrow / nlvr2_test1.arrow ->
nlvr2_dataset.npz, tools/gen_golden_nlvr2.py dataset): index, statements, answers as bools, table names and both image views; and the
collate of a pair batch (image_0 / image_1 padded to one shared extent, answers / table_name as lists)."""
import os

import numpy as np

import rmcl_pkg  # noqa: F401
from rmcl_amd.attack import word_substitution as WS
from rmcl_amd.vilt.datasets import NLVR2Dataset, collate
from tests.golden_util import digest, load

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dataset():
    return NLVR2Dataset(GOLD, ["pixelbert"], 64, split="val", tokenizer=WS.load_tokenizer(os.path.join(GOLD, "toy_vocab.txt")))


def test_nlvr2_dataset_matches_reference():
    g = load("nlvr2_dataset.npz")
    ds = _dataset()
    assert len(ds) == int(g["len"])
    np.testing.assert_array_equal(np.array([list(ds.index_mapper[j]) for j in range(len(ds))]), g["index_mapper"])
    for j in range(len(ds)):
        r = ds[j]
        assert r["text"][0] == str(g[f"s{j}_text"]) and list(r["text"][1]["input_ids"]) == g[f"s{j}_ids"].tolist()
        assert isinstance(r["answers"], bool) and int(r["answers"]) == int(g[f"s{j}_answers"])
        assert r["table_name"] == str(g[f"s{j}_table_name"])
        for k in ("image_0", "image_1"):
            assert tuple(r[k][0].shape) == tuple(g[f"s{j}_{k}_shape"].tolist())
            np.testing.assert_allclose(digest(r[k][0]), g[f"s{j}_{k}_digest"], rtol=1e-6, atol=1e-5)


def test_nlvr2_collate_pads_both_images_to_one_extent():
    ds = _dataset()
    b = collate([ds[j] for j in range(len(ds))])
    i0, i1 = b["image_0"][0], b["image_1"][0]
    assert i0.shape == i1.shape and i0.shape[0] == len(ds)
    assert b["answers"] == [ds[j]["answers"] for j in range(len(ds))]
    assert [("dev" in n, "test" in n) for n in b["table_name"]] == [(True, False)] * 3 + [(False, True)] * 3
    assert tuple(b["text_ids"].shape) == (len(ds), 40)
