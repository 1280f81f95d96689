"""CPU: the reference, the two rounding models and the inputs of tests/test_infonce_kernels_gpu.py, on their own.

The GPU tests allow a kernel 4 x model_f32's (fp32 arms) or 3 x model_split's (split arms) worst-row figure on the same case.  The caps
here keep that from becoming a loose absolute bound: per input family and output, each model's worst figure over the whole case list
must stay within 1.5 x MEASURED below - MEASURED is that worst figure as measured on the CPU (two digits; "f32": the worse of the
two summation orders of model_f32), the factor 1.5 is for another BLAS summation order; 1.5 * MEASURED is what is asserted.  What the table says about the kernel's formula:
  * loss_i / lse err against S_i = max |logit| sits at 5e-7 .. 8e-7 in fp32 and at 5e-6 .. 8e-6 with split products;
  * dq per row is 1e-5 .. 3e-5 in fp32 on the randn queue (a 2e-5 absolute logit error at |l| = 60 is a 2e-5 relative error of p) and
    2e-4 with split products; on `trained` and `dup_pos` it is 1e-4 .. 4e-4 (1.4e-3 split) because the formula takes
    (p_pos - 1) k + sum_j p_j key_j with p_pos = epos / Z close to 1: the small-gradient rows the whole-tensor figure never saw;
  * the split model's logit error, relative to |q| |c| / T, is 2.6e-6 at worst: inside the header's 2^-16 = 1.5e-5.
Also asserted, because the GPU tests rely on it: every (arm, B, Kq) of the case list satisfies the launch condition of its arm (the arm
table of the GPU file's docstring, written down again below, against launched()); `trained` has the positive as arg-max in every
row; the spike and tie placements win in fp64 (a planted twin never does); the rows whose fp64 top-two gap is below 4 x a model's
logit error are exactly the dup_pos rows placed; metric_rows() has the batch means of oracle.queue_metrics."""
import pytest
import torch

from oracle import rmcl_oracle as O
from tests.test_infonce_kernels_gpu import (ALL, ARMS, BASE, KQS, OUTS, Case, analysis, inputs, launched, metric_rows, near_ties,
                                            spike_pairs, tie_triples)

MEASURED = {
    ("randn", "f32"): {"dq": 1.2e-05, "l_pos": 1.3e-08, "logit_rel": 2.7e-07, "loss_i": 5.2e-07, "lse": 5.4e-07, "neg_cos": 6.5e-09, "neg_dist": 1.8e-07, "neg_dot": 5.4e-08, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
    ("randn", "split"): {"dq": 0.00013, "l_pos": 1.3e-08, "logit_rel": 2.6e-06, "loss_i": 5.2e-06, "lse": 5.2e-06, "neg_cos": 5.5e-08, "neg_dist": 2.2e-07, "neg_dot": 6.6e-07, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
    ("spikes", "f32"): {"dq": 2.4e-05, "l_pos": 1.1e-08, "logit_rel": 3e-07, "loss_i": 6.8e-07, "lse": 6.8e-07, "neg_cos": 5.7e-09, "neg_dist": 1.8e-07, "neg_dot": 9.6e-08, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
    ("spikes", "split"): {"dq": 0.00019, "l_pos": 9.2e-09, "logit_rel": 2.6e-06, "loss_i": 6.8e-06, "lse": 6.8e-06, "neg_cos": 5.9e-08, "neg_dist": 1.6e-07, "neg_dot": 7.2e-07, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
    ("ties", "f32"): {"dq": 2.6e-05, "l_pos": 1.3e-08, "logit_rel": 3e-07, "loss_i": 7.5e-07, "lse": 7.5e-07, "neg_cos": 5.4e-09, "neg_dist": 2.1e-07, "neg_dot": 7.4e-08, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
    ("ties", "split"): {"dq": 0.0002, "l_pos": 1.3e-08, "logit_rel": 2.6e-06, "loss_i": 6.5e-06, "lse": 6.5e-06, "neg_cos": 5.5e-08, "neg_dist": 1.9e-07, "neg_dot": 7.5e-07, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
    ("trained", "f32"): {"dq": 8.8e-05, "l_pos": 1.1e-07, "logit_rel": 2.2e-07, "loss_i": 6.7e-07, "lse": 5.3e-07, "neg_cos": 6e-09, "neg_dist": 2.3e-07, "neg_dot": 5.7e-09, "pos_cos": 1.6e-07, "pos_dist": 4.9e-08, "pos_dot": 9.1e-08},
    ("trained", "split"): {"dq": 4.8e-05, "l_pos": 1.1e-07, "logit_rel": 2.3e-06, "loss_i": 5.9e-07, "lse": 5.7e-07, "neg_cos": 5.9e-08, "neg_dist": 2.3e-07, "neg_dot": 5.9e-08, "pos_cos": 1.6e-07, "pos_dist": 4.9e-08, "pos_dot": 9.1e-08},
    ("dup_pos", "f32"): {"dq": 0.00038, "l_pos": 1.1e-07, "logit_rel": 2.2e-07, "loss_i": 1.1e-07, "lse": 1.4e-07, "neg_cos": 6.2e-09, "neg_dist": 2.2e-07, "neg_dot": 6.1e-09, "pos_cos": 1.6e-07, "pos_dist": 4.9e-08, "pos_dot": 9.1e-08},
    ("dup_pos", "split"): {"dq": 0.0014, "l_pos": 1.1e-07, "logit_rel": 2.3e-06, "loss_i": 6.7e-07, "lse": 6.1e-07, "neg_cos": 5.8e-08, "neg_dist": 2e-07, "neg_dot": 5.8e-08, "pos_cos": 1.6e-07, "pos_dist": 4.9e-08, "pos_dot": 9.1e-08},
    ("mixed", "f32"): {"dq": 1.3e-05, "l_pos": 1.5e-08, "logit_rel": 2.3e-07, "loss_i": 5.8e-07, "lse": 5.5e-07, "neg_cos": 5.7e-09, "neg_dist": 1.7e-07, "neg_dot": 4e-08, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
    ("mixed", "split"): {"dq": 0.00013, "l_pos": 1.3e-08, "logit_rel": 2.3e-06, "loss_i": 3.6e-06, "lse": 3.6e-06, "neg_cos": 6.1e-08, "neg_dist": 2.6e-07, "neg_dot": 4.5e-07, "pos_cos": 5.2e-08, "pos_dist": 7.4e-08, "pos_dot": 2.8e-08},
}
CAP_FACTOR = 1.5
HEADER_CLAIM = 2.0 ** -16           # infonce.hip: the split product's error relative to |q| |c| (/ T for a logit)
CASES = list(dict.fromkeys(case for _, case in ALL))

# the arm table of the issue / the GPU file's docstring: arm -> (entry, with_metrics, key 5, Kq % 256 it takes, kernels)
ARM_TABLE = {"f32_fold": ("f32", 1, 1, (0,), ("partial2", "combine2")),
             "f32_odd": ("f32", 1, 1, (128,), ("partial", "combine2")),
             "f32_round1": ("f32", 1, 0, (0, 128), ("partial", "combine")),
             "split_m1": ("split", 1, 1, (0,), ("partial3<true>", "combine2")),
             "split_m0": ("split", 0, 1, (0,), ("partial3<false>", "combine2")),
             "split_fallback_m1": ("split", 1, 1, (128,), ("partial", "combine2")),
             "split_fallback_m0": ("split", 0, 1, (128,), ("partial", "combine2"))}


def test_every_case_satisfies_the_launch_condition_of_its_arm():
    assert set(ARM_TABLE) == set(ARMS)
    for arm, (entry, wm, key5, residues, kernels) in ARM_TABLE.items():
        assert ARMS[arm][:4] == (entry, wm, key5, kernels)
        for Kq in KQS + (512,):
            assert (launched(entry, wm, key5, Kq)[:2] == kernels) == (Kq % 256 in residues), (arm, Kq)
    for arm, case in ALL:
        assert case.Kq % 256 in ARM_TABLE[arm][3] and launched(*ARMS[arm][:3], case.Kq)[:2] == ARMS[arm][3], (arm, case)
    # partials per row that the shapes were chosen for: below, at and above the combine's 8 slice groups, 129 and 256 (batch fetch), 512
    assert [launched("f32", 1, 1, Kq)[2] for Kq in KQS] == [1, 1, 3, 8, 17, 9, 129, 256]
    assert launched("f32", 1, 0, 65536)[2] == 512
    for arm in ARMS:                                           # every B at one Kq, every accepted Kq at B = 65, T = 1 once
        shapes = {(c.B, c.Kq) for a, c in ALL if a == arm}
        assert {B for B, Kq in shapes if Kq == ARMS[arm][4]} == {1, 4, 63, 64, 65, 130}
        assert {Kq for B, Kq in shapes if B == 65} >= {Kq for Kq in KQS if Kq % 256 in ARM_TABLE[arm][3]}
        assert all(B in (4, 65) for B, Kq in shapes if Kq >= 33024)
        assert any(c.T == 1.0 for a, c in ALL if a == arm)


def test_placements_reach_the_boundaries():
    assert {j for _, j in spike_pairs(65, 512)} == {511, 0, 63, 64, 127, 128, 255, 256}
    assert [r for r, _ in spike_pairs(65, 512)][:2] == [64, 0]                   # the one row of the second tile
    assert [r for r, _ in spike_pairs(130, 512)][:2] == [129, 64]             # last row of the ragged third tile, first row of the second
    assert spike_pairs(1, 128) == [(0, 127)]
    t = tie_triples(65, 65536)
    assert all(j1 < j2 for _, j1, j2 in t)
    assert any(j1 // 64 == j2 // 64 and j1 % 4 > j2 % 4 for _, j1, j2 in t)                    # one sub-slice, the later column in an earlier lane
    assert any(j1 // 256 == j2 // 256 and j1 // 64 != j2 // 64 for _, j1, j2 in t)           # sub-slices of one workgroup
    assert any(j2 // 256 >= 64 and j1 // 256 == 0 for _, j1, j2 in t)                          # the combine's second wave
    j1, j2 = tie_triples(65, 33024)[0][1:]
    assert (j2 // 256) % 128 == (j1 // 256) % 128 and j2 // 256 == 128                         # one combine thread, two trips of its loop


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-B{}-Kq{}-T{}".format(*c))
def test_models_and_inputs(case):
    a = analysis(case)
    info = inputs(case)[3]
    assert set(a.fig) == ({"f32_128", "f32_256", "split"} if case.Kq % 256 == 0 else {"f32_128"})
    for kind in a.fig:
        cap = MEASURED[(case.family, kind[:3] if kind != "split" else kind)]
        over = {n: (a.fig[kind][n], CAP_FACTOR * cap[n]) for n in OUTS if not a.fig[kind][n] <= CAP_FACTOR * cap[n]}
        assert not over, (kind, over)
        assert a.logit_err[kind + "_rel"] <= CAP_FACTOR * cap["logit_rel"], (kind, a.logit_err)
        near = near_ties(case, kind)
        assert near.nonzero().flatten().tolist() == sorted(info["dups"]), (kind, float(a.gap.min()), a.logit_err[kind])
    assert a.logit_err.get("split_rel", 0.0) <= HEADER_CLAIM
    assert (case.family == "dup_pos") == bool(info["dups"]) and (case.family in ("spikes", "ties")) == bool(info["winners"])
    for r, want in info["winners"].items():
        assert int(a.argmax[r]) == want, (r, int(a.argmax[r]), want)
    assert not any(int(j) - 1 in info["twins"] for j in a.argmax), "a planted twin wins in fp64"
    if BASE[case.family] == "trained":
        others = [r for r in range(case.B) if r not in info["dups"]]
        assert bool((a.argmax[others] == 0).all()), "trained: the positive is not the arg-max of every row"
    if case.family in ("randn", "mixed"):                      # the data of the old tests: the positive never wins there
        assert bool((a.argmax != 0).all())


@pytest.mark.parametrize("family", ["randn", "trained", "mixed"])
def test_metric_rows_have_the_oracles_batch_means(family):
    q, k, queue, _ = inputs(Case(family, 65, 384, 0.07))
    rows = metric_rows(q.double(), k.double(), queue.double())
    m = O.queue_metrics(q.double(), k.double(), queue.double())
    for n, name in (("pos_dist", "pos_dist"), ("pos_cos", "pos_cosine"), ("pos_dot", "pos_dot"), ("neg_dist", "neg_dist"), ("neg_cos", "neg_cosine"),
                    ("neg_dot", "neg_dot")):
        assert abs(float(rows[n].mean()) - float(m[name])) <= 1e-13 * max(1.0, abs(float(m[name]))), n
