"""-m gpu: rmcl_infonce_f32 / rmcl_infonce_split_bf16 against float64, row by row, at every launch arm of csrc/infonce.hip.

Arms (launched() below writes the launch conditions of rmcl_infonce down once; every case asserts the arm it is named after).
  arm             entry                                  key 5   Kq              kernels
  f32_fold        rmcl_infonce_f32                       1       % 256 == 0      partial2 + combine2
  f32_odd         rmcl_infonce_f32                       1       % 256 == 128    partial + combine2
  f32_round1      rmcl_infonce_f32                       0       % 128 == 0      partial + combine
  split_m1        rmcl_infonce_split_bf16, metrics 1     1       % 256 == 0      partial3<true> + combine2
  split_m0        rmcl_infonce_split_bf16, metrics 0     1       % 256 == 0      partial3<false> + combine2
  split_fallback  rmcl_infonce_split_bf16, metrics 1, 0  1       % 256 == 128    partial + combine2 (the exact-f32 kernel)
rmcl_tune_set key 5 is put back to 1 in a `finally`.

Shapes.  B in {1, 4, 63, 64, 65, 130} (one, two, three row tiles of RT = 64, ragged last tiles) at one small Kq per arm; at B = 65 every
Kq of {128, 256, 384, 2048, 2176, 2304, 33024, 65536} the arm accepts (128: one slice, fewer slices than the combine's 8 slice groups;
256: one folded workgroup; 384: the odd arm with 3 slices; 2048: 8 partials; 2176 = 128 * 17: the odd arm with more slices than groups;
2304: 9 partials, one group with two; 33024 = 256 * 129: the second trip of the combine's `s += PD` loop; 65536: the batch-fetch arm
(256 partials) under key 5 = 1, 512 slices under key 5 = 0); Kq >= 33024 at B = 4 and B = 65 only.  Temperature 0.07 everywhere, 1.0
once per arm and base family; grad_scale = 1 / (3 B).

Input families (CPU generators, fixed seeds; q is unit-norm): `randn` (un-normalised randn queue, k = normalize(randn + 2 q): logits
to +-60), `trained` (unit queue columns, k = normalize(q + 0.05 randn): the positive is the arg-max of every row), `mixed` (first half
of the queue unit-norm, the rest randn), `spikes` (randn; queue column j* = 30 q[r] for (r, j*) at the first and last column and on
both sides of the 64-, 128- and 256-column boundaries, r including the last row of a ragged tile and the first row of the second tile:
a logit of 428 that the running-max rescaling must survive), `ties` (randn; two bit-identical columns j1 < j2 = 30 q[r]: in one
64-column sub-slice in different `t & 3` lanes, in different sub-slices, in different workgroups, the far one in the last workgroup -
pred must be j1 + 1), `dup_pos` (trained; one queue column equals k[r]: the positive and that column tie up to the summation route).

Reference.  float64 on the fp32 values the kernel reads: oracle.rmcl_oracle.infonce_logits / infonce_loss, autograd for dq, and
metric_rows() - oracle.queue_metrics kept per row (tests/test_infonce_model_cpu.py holds its batch means to the oracle's).

Models (plain torch, CPU).  model_f32: the header formula of infonce.hip in fp32 - logits, softmax, dq = g/T (sum_j p_j key_j - k_i),
metrics in the expanded form sqrt(max(qq + cc - 2 dot, 0)).  model_split: q and the queue split as the kernel splits them (hi = bf16(x),
lo = bf16(x - hi)), logits = hi.hi + hi.lo + lo.hi; for dq the kernel splits BOTH factors again: P of a 64-column sub-slice, taken
relative to the running maximum of its 256-column workgroup (exp(l - max_sub) * exp(max_sub - max_run), the value partial3 feeds the
matrix cores), is split hi / lo and multiplied with the split queue as Qhi.Phi + Qhi.Plo + Qlo.Phi; the rescaling to the row maximum,
Z, the positive (an exact fp32 dot product in the combine kernel) and all metrics but the dots are fp32.
Both models take the SUMS that are single fp32 roundings next to their bound in the kernels' own order - the four 128-term sums of the
positive pair (wave_sum's butterfly, wave 0 + wave 1), the squared query norm and the squared column norms as each partial kernel
forms them (a serial fma walk in infonce_partial_kernel; float4 partials and a 32-lane butterfly for q, a thread's 8 rows by fma,
the butterfly over its 4 row groups and the 4 waves for the columns in the folded forms), and the three queue means (a thread's
serial walk over its columns, the 4-thread butterfly, the combine thread's serial walk over its slices, wave_sum) - so model_f32
exists per partial-kernel width (128 / 256 columns per workgroup).  A pairwise torch sum is more accurate than the kernel can be: with
plain sums 3 x model sat below one ulp of l_pos and neg_dist at B = 1 and 4 (six cases), with the column norms alone left as a plain sum
below one ulp of neg_dist at (trained, B = 4, Kq = 33024) - kernel 9.31e-08 against 8.99e-08.  That the orders above are the kernels' was
checked against the figures the kernels gave: with the fma walk of the column norms the model's neg_cos figure equals the kernel's to
three digits in 51 of 69 f32_fold cases (5 of 69 with a plain sum), neg_dist in 66 of 69; l_pos and the failing neg_dist figures are
reproduced digit for digit.  The matrix products and Z stay plain torch products and sums: what the matrix cores' accumulation order
leaves is a dot-product noise of 1e-8 that no model on the CPU reproduces, so a split-arm figure at the level of one ulp (no floor in
that bound) can still move by one ulp between the kernel and the model.

Metric, per row, asserted on the MAXIMUM over rows:
  loss_i, l_pos, lse : |d| / S_i, S_i = max(1, max_j |logit_ij|)   (both lse and l_pos are single roundings at that magnitude)
  dq                 : |got_i - ref_i|_2 / max(|ref_i|_2, 0.05 * rms row norm); the old global max|d| / max|ref| is recorded next to it
  the six metrics    : |d| / max(1, |ref|)
  pred               : equal to argmax of the fp64 logits (first index wins) on every row whose fp64 top-two gap is at least 4 x the
                       model's worst logit error of the case (for a planted tie: the gap to the next different column); the
                       number of rows left out must equal the dup_pos rows placed.
  loss_sum           : started at c0 = 0.75; c0 + mean_i loss_i within 4 * 2^-24 * max(|c0|, max_i |loss_i|) + the row bound * max_i S_i.
Bound.  fp32 arms, split_fallback included: err <= 4 * max(e32, 2^-23), e32 the same figure of model_f32 on the same case.
Split arms: err <= 3 * max(model_split's figure, e32).  (The factors of the earlier pins; nothing new.)
Measured on an MI355X (profiles/infonce_parity.json): over the 489 arm cases the largest kernel / allowed ratio is 0.67 (dq, f32_fold,
mixed-B1-Kq512), 0.47 on the one-slice arms and 0.60 on the split arms (lse at T = 1).

Contract, every run of every case: dq, rows_out, loss_sum and a workspace of exactly rmcl_infonce_ws_bytes(B, Kq) bytes lie between
guard bytes, pre-filled with NaN; the guards are intact afterwards, dq and rows_out hold no NaN, q / k / queue are bit-unchanged; a
second identical call (loss_sum = NULL) gives the same bits in rows_out and dq; a third with dq = NULL gives the same rows_out bits and
adds the mean loss to loss_sum once more (`+=`); with_metrics = 0 writes rows_out[:, 6:9] = 0 exactly on every arm, the fallback included.

Measured figures, kernel next to model and allowed, go to the file named by RMCL_INFONCE_PARITY_OUT when set
(profiles/infonce_parity.json is such a dump).
"""
import collections
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rmcl_oracle as O  # noqa: E402
from tests.gpu_util import DEV, lib, check, P, I64, F, stream  # noqa: E402
from tests.test_attention_kernels_gpu import Guarded, bits, bf  # noqa: E402

Case = collections.namedtuple("Case", "family B Kq T")
PD, RT, CMB_G = 128, 64, 8
SCALARS = ("loss_i", "l_pos", "lse")
METRICS = ("pos_dist", "pos_cos", "pos_dot", "neg_dist", "neg_cos", "neg_dot")      # rows_out[:, 3:9]
OUTS = SCALARS + ("dq",) + METRICS
F32_FACTOR, F32_FLOOR, SPLIT_FACTOR = 4.0, 2.0 ** -23, 3.0
C0 = 0.75
QUEUE_SEED = 4                      # (q: 1, k: 2, as tests/test_kernels_gpu.py) - a seed at which no case has a near-tie of its own (CPU test)
BASE = {"randn": "randn", "spikes": "randn", "ties": "randn", "trained": "trained", "dup_pos": "trained", "mixed": "mixed"}
FAMILIES = tuple(BASE)
BS = (1, 4, 63, 64, 65, 130)
KQS = (128, 256, 384, 2048, 2176, 2304, 33024, 65536)
# arm -> (entry, with_metrics, rmcl_tune_set key 5, kernels, the arm's own small Kq)
ARMS = {"f32_fold": ("f32", 1, 1, ("partial2", "combine2"), 512),
        "f32_odd": ("f32", 1, 1, ("partial", "combine2"), 384),
        "f32_round1": ("f32", 1, 0, ("partial", "combine"), 384),
        "split_m1": ("split", 1, 1, ("partial3<true>", "combine2"), 512),
        "split_m0": ("split", 0, 1, ("partial3<false>", "combine2"), 512),
        "split_fallback_m1": ("split", 1, 1, ("partial", "combine2"), 384),
        "split_fallback_m0": ("split", 0, 1, ("partial", "combine2"), 384)}
MODEL_KINDS = ("f32_128", "f32_256", "split")                  # model_f32 in the summation order of partial / partial2, model_split
PARITY = {}


def launched(entry, with_metrics, key5, Kq):
    """The launch conditions of rmcl_infonce: (partial kernel, combine kernel, partials per row)."""
    assert Kq > 0 and Kq % 128 == 0
    fold = key5 >= 1 and Kq % 256 == 0
    if entry == "split" and fold:
        part = "partial3<true>" if with_metrics else "partial3<false>"
    else:
        part = "partial2" if fold else "partial"
    return part, "combine2" if key5 >= 1 else "combine", Kq // 256 if fold else Kq // 128


def accepts(arm, Kq):
    entry, wm, key5, kernels, _ = ARMS[arm]
    return launched(entry, wm, key5, Kq)[:2] == kernels


def arm_cases(arm):
    """Every B at the arm's small Kq, every accepted Kq at B = 65, the large Kq at B = 4 too; T = 1 once per base family."""
    small = ARMS[arm][4]
    shapes = [(B, small) for B in BS] + [(65, Kq) for Kq in KQS if accepts(arm, Kq) and Kq != small]
    shapes += [(4, Kq) for Kq in KQS if accepts(arm, Kq) and Kq >= 33024]
    cases = [Case(f, B, Kq, 0.07) for B, Kq in shapes for f in FAMILIES]
    return cases + [Case(f, 65, small, 1.0) for f in ("randn", "trained", "mixed")]


ALL = [(arm, case) for arm in ARMS for case in arm_cases(arm)]


def case_id(v):
    return v if isinstance(v, str) else "{}-B{}-Kq{}-T{}".format(*v)


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("RMCL_INFONCE_PARITY_OUT")
    if out and PARITY:
        worst = max((v[3], f"{c}:{a}:{o}") for c, arms in PARITY.items() for a, fig in arms.items() for o, v in fig.items() if o in OUTS)
        head = {"columns": ["kernel_worst_row", "model_worst_row", "allowed_worst_row", "kernel_over_allowed"],
                "dq_global": ["kernel max|d|/max|ref|", "model max|d|/max|ref|"],
                "model": "f32 arms and split_fallback: model_f32; split_m1 / split_m0: model_split (allowed = 3 * max(model_split, model_f32))",
                "largest_kernel_over_allowed": worst[0], "largest_at": worst[1]}
        with open(out, "w") as f:                              # one line per case and arm
            f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()) + ' "cases": {\n')
            f.write(",\n".join(f"  {json.dumps(c)}: {{" + ", ".join(f"{json.dumps(a)}: {json.dumps(fig)}" for a, fig in sorted(arms.items())) + "}"
                               for c, arms in sorted(PARITY.items())))
            f.write("\n }\n}\n")


# ------------------------------------------------------------------------------------------ inputs (CPU)
def unit_rows(x):
    return x / x.norm(dim=1, keepdim=True)


def spike_pairs(B, Kq):
    """(row, column): the column order puts the edges first, the row order the last row (of a ragged tile), the first of tile 2, then 0.."""
    cols = [j for j in dict.fromkeys((Kq - 1, 0, 63, 64, 127, 128, 255, 256)) if 0 <= j < Kq]
    rows = list(dict.fromkeys([B - 1] + ([64] if B > 64 else []) + list(range(B))))
    return list(zip(rows, cols))


def tie_triples(B, Kq):
    """(row, j1, j2), j1 < j2: far apart in different workgroups (j2 in the last one), in one sub-slice with lane(j1) = 3 > lane(j2) = 0,
    in neighbouring sub-slices, in sub-slices 1 and 3 of a 256-column workgroup (= two 128-column slices)."""
    places = ([(130, Kq - 3)] if Kq >= 384 else []) + [(7, 12), (20, 84)] + ([(70, 200)] if Kq >= 256 else [])
    return [(r, j1, j2) for r, (j1, j2) in enumerate(places) if r < B]


def dup_pairs(B, Kq):
    return [(0, 3)] + ([(B - 1, Kq - 1)] if B > 1 else [])


@functools.lru_cache(maxsize=2)
def inputs(case):
    """fp32 q [B, 128], k [B, 128], queue [128, Kq] on the CPU and {"winners": {row: pred}, "dups": [rows]}."""
    family, B, Kq, _ = case
    gen = lambda seed: torch.Generator(device="cpu").manual_seed(seed)
    q = unit_rows(torch.randn(B, PD, generator=gen(1)))
    noise = torch.randn(B, PD, generator=gen(2))
    queue = torch.randn(PD, Kq, generator=gen(QUEUE_SEED))
    base = BASE[family]
    if base == "trained":
        k = unit_rows(q + 0.05 * noise)
        queue = queue / queue.norm(dim=0, keepdim=True)
    else:
        k = unit_rows(noise + 2 * q)
        if base == "mixed":
            queue[:, :Kq // 2] = queue[:, :Kq // 2] / queue[:, :Kq // 2].norm(dim=0, keepdim=True)
    info = {"winners": {}, "dups": [], "twins": []}
    if family == "spikes":
        for r, j in spike_pairs(B, Kq):
            queue[:, j] = 30 * q[r]
            info["winners"][r] = j + 1
    elif family == "ties":
        for r, j1, j2 in tie_triples(B, Kq):
            queue[:, j1] = 30 * q[r]
            queue[:, j2] = queue[:, j1]
            info["winners"][r] = j1 + 1
            info["twins"].append(j2)
    elif family == "dup_pos":
        for r, j in dup_pairs(B, Kq):
            queue[:, j] = k[r]
            info["dups"].append(r)
    return q.contiguous(), k.contiguous(), queue.contiguous(), info


# ------------------------------------------------------------------------------------------ reference and models (CPU)
def metric_rows(q, k, queue, dots=None):
    """oracle.queue_metrics per row instead of per batch, in the dtype of its arguments (the expanded distance of the kernel)."""
    qq, cc = (q * q).sum(1, keepdim=True), (queue * queue).sum(0)[None]
    dots = q @ queue if dots is None else dots
    dotp = (q * k).sum(1)
    return {"pos_dist": (q - k).norm(dim=1), "pos_cos": dotp / (qq[:, 0].sqrt() * (k * k).sum(1).sqrt()).clamp_min(1e-6), "pos_dot": dotp,
            "neg_dist": (qq + cc - 2 * dots).clamp_min(0).sqrt().mean(1), "neg_cos": (dots / (qq.sqrt() * cc.sqrt()).clamp_min(1e-6)).mean(1),
            "neg_dot": dots.mean(1)}


def reference_of(q, k, queue, T, gscale):
    """float64: the outputs per row, the logits [B, 1 + Kq]."""
    qd = q.double().requires_grad_(True)
    kd, cd = k.double(), queue.double()
    logits = O.infonce_logits(qd, kd, cd, T)
    (O.infonce_loss(logits) * (gscale * q.shape[0])).backward()
    logits = logits.detach()
    lse = torch.logsumexp(logits, 1)
    ref = {"loss_i": lse - logits[:, 0], "l_pos": logits[:, 0], "lse": lse, "dq": qd.grad}
    ref.update(metric_rows(qd.detach(), kd, cd))
    return ref, logits


def split2(x):
    hi = bf(x)
    return hi, bf(x - hi)


def wave_sum(x):
    """rmcl_common.h wave_sum over a last dimension of 64 lanes: the xor butterfly, o = 32 .. 1."""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lanes ^ o]
    return x[..., 0]


def dot128(a, b):
    """The combine kernels' 128-term sums of the positive pair: one product per thread, wave_sum, wave 0 + wave 1."""
    w = wave_sum((a * b).view(-1, 2, 64))
    return w[:, 0] + w[:, 1]


def fma(a, b, c):
    """fp32 a * b + c with one rounding (the product of two floats is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def query_norms(q, width):
    """Squared query norms as the partial kernels form them: a serial fma walk (one slice per workgroup), or float4 partials and a
    butterfly over the 32 lanes of a row (folded forms)."""
    if width == 128:
        s = torch.zeros(q.shape[0])
        for c in range(PD):
            s = fma(q[:, c], q[:, c], s)
        return s
    x = q.view(-1, 32, 4)
    sq = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + (x[..., 2] * x[..., 2] + x[..., 3] * x[..., 3])
    lanes = torch.arange(32)
    for o in (1, 2, 4, 8, 16):
        sq = sq + sq[:, lanes ^ o]
    return sq[:, 0]


def column_norms(queue, width):
    """Squared queue-column norms as the partial kernels form them, `s += v * v` contracted to an fma: a serial walk down the 128 rows
    (one slice per workgroup), or - folded forms, `deposit` - a thread's rows c = 16 i + 4 wave + g serially over i, the butterfly over
    g, then (wave 0 + wave 1) + (wave 2 + wave 3)."""
    Kq = queue.shape[1]
    if width == 128:
        s = torch.zeros(Kq)
        for c in range(PD):
            s = fma(queue[c], queue[c], s)
        return s
    x = queue.view(8, 4, 4, Kq)                                # [i, wave, g, column]
    acc = torch.zeros(4, 4, Kq)
    for i in range(8):
        acc = fma(x[i], x[i], acc)
    w = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    return (w[0] + w[1]) + (w[2] + w[3])


def queue_mean(v, width):
    """Mean over the queue of v [B, Kq] in the kernels' order: a thread (column % 4) of a row adds its columns of a workgroup serially
    (sub-slice by sub-slice), the 4 threads meet in a butterfly, combine thread s % 128 adds the partials of its slices serially, then
    wave_sum and wave 0 + wave 1, / Kq."""
    B, Kq = v.shape
    t = v.view(B, Kq // width, width // 4, 4)
    acc = torch.zeros(B, Kq // width, 4)
    for i in range(width // 4):
        acc = acc + t[:, :, i]
    part = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    n = part.shape[1]
    part = torch.cat([part, torch.zeros(B, -n % PD)], 1).view(B, -1, PD)
    thr = torch.zeros(B, PD)
    for i in range(part.shape[1]):
        thr = thr + part[:, i]
    w = wave_sum(thr.view(B, 2, 64))
    return (w[:, 0] + w[:, 1]) / torch.tensor(float(Kq), dtype=torch.float32)


def model_metrics(q, k, queue, dots, dotp, width):
    """rows_out[:, 3:9] in fp32 with the kernels' summation orders."""
    qq_c, kk = dot128(q, q), dot128(k, k)
    qq, cc = query_norms(q, width)[:, None], column_norms(queue, width)[None]
    return {"pos_dist": dot128(q - k, q - k).sqrt(), "pos_cos": dotp / (qq_c.sqrt() * kk.sqrt()).clamp_min(1e-6), "pos_dot": dotp,
            "neg_dist": queue_mean((qq + cc - 2.0 * dots).clamp_min(0).sqrt(), width),
            "neg_cos": queue_mean(dots / (qq.sqrt() * cc.sqrt()).clamp_min(1e-6), width), "neg_dot": queue_mean(dots, width)}


def model_of(q, k, queue, T, gscale, split, width):
    """model_f32 (split = False) / model_split (True) of the docstring for the partial kernel with `width` queue columns per workgroup
    (128: infonce_partial_kernel, 256: the folded forms): fp32 outputs per row and the logits [B, 1 + Kq]."""
    B, Kq = q.shape[0], queue.shape[1]
    invT = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32)
    dotp = dot128(q, k)
    if split:
        qh, ql = split2(q)
        ch, cl = split2(queue)
        dots = qh @ ch + qh @ cl + ql @ ch
    else:
        dots = q @ queue
    lpos, lneg = dotp * invT, dots * invT
    M = torch.maximum(lneg.amax(1), lpos)
    epos = torch.exp(lpos - M)
    if split:
        l4 = lneg.view(B, Kq // 256, 4, 64)
        ms = l4.amax(3)                                        # sub-slice maxima, the running maximum inside a workgroup
        mr = ms.cummax(2).values
        p = torch.exp(l4 - ms[..., None]) * torch.exp(ms - mr)[..., None]
        ph, pl = split2(p)
        h4, c4 = ch.view(PD, Kq // 256, 4, 64), cl.view(PD, Kq // 256, 4, 64)
        prod = torch.einsum("bwsj,cwsj->bwsc", ph, h4) + torch.einsum("bwsj,cwsj->bwsc", pl, h4) + torch.einsum("bwsj,cwsj->bwsc", ph, c4)
        f = torch.exp(mr - M[:, None, None])
        acc = (prod * f[..., None]).sum((1, 2))
        Z = (p.sum(3) * f).sum((1, 2)) + epos
    else:
        p = torch.exp(lneg - M[:, None])
        acc = p @ queue.t()
        Z = p.sum(1) + epos
    lse = torch.log(Z) + M
    mod = {"loss_i": lse - lpos, "l_pos": lpos, "lse": lse, "dq": gscale * invT * ((epos / Z - 1.0)[:, None] * k + acc / Z[:, None])}
    mod.update(model_metrics(q, k, queue, dots, dotp, width))
    return mod, torch.cat([lpos[:, None], lneg], 1)


def row_err(got, ref):
    got, ref = got.double(), ref.double()
    rn = ref.norm(dim=1)
    return float(((got - ref).norm(dim=1) / rn.clamp_min(0.05 * float(rn.square().mean().sqrt()))).max())


def glob_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def figures(got, ref, S):
    """{output: worst-row error}, "dq_global": the whole-tensor figure of tests/test_kernels_gpu.py."""
    fig = {n: float(((got[n].double() - ref[n]).abs() / S).max()) for n in SCALARS}
    fig["dq"] = row_err(got["dq"], ref["dq"])
    fig.update({n: float(((got[n].double() - ref[n]).abs() / ref[n].abs().clamp_min(1.0)).max()) for n in METRICS})
    fig["dq_global"] = glob_err(got["dq"], ref["dq"])
    return fig


Analysis = collections.namedtuple("Analysis", "ref S argmax gap fig logit_err")


@functools.lru_cache(maxsize=None)
def analysis(case):
    """Reference, the models' figures {"f32_128" | "f32_256" | "split": ...} (the latter two where Kq % 256 == 0: where those kernels run)
    and their worst logit errors for one case; keeps only per-row tensors."""
    q, k, queue, info = inputs(case)
    gscale = 1.0 / (3.0 * case.B)
    ref, logits = reference_of(q, k, queue, case.T, gscale)
    S = logits.abs().amax(1).clamp_min(1.0)
    distinct = logits.clone()                                  # a planted pair is one value twice in EVERY row: the gap is taken without j2
    distinct[:, [1 + j2 for j2 in info["twins"]]] = float("-inf")
    top = distinct.topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    fig, lerr = {}, {}
    for kind in MODEL_KINDS if case.Kq % 256 == 0 else MODEL_KINDS[:1]:
        mod, ml = model_of(q, k, queue, case.T, gscale, kind == "split", 128 if kind == "f32_128" else 256)
        fig[kind] = figures(mod, ref, S)
        lerr[kind] = float((ml.double() - logits).abs().max())
        lerr[kind + "_rel"] = float(((ml[:, 1:].double() - logits[:, 1:]).abs() * case.T / (q.double().norm(dim=1)[:, None] * queue.double().norm(dim=0)[None])).max())
    return Analysis(ref, S, logits.argmax(1), gap, fig, lerr)


def model_kind(arm, Kq):
    return {"partial": "f32_128", "partial2": "f32_256"}.get(launched(*ARMS[arm][:3], Kq)[0], "split")


def allowed_figures(case, arm):
    a = analysis(case)
    kind = model_kind(arm, case.Kq)
    if kind == "split":
        return {n: SPLIT_FACTOR * max(a.fig["split"][n], a.fig["f32_256"][n]) for n in OUTS}
    return {n: F32_FACTOR * max(a.fig[kind][n], F32_FLOOR) for n in OUTS}


def near_ties(case, kind):
    """Rows whose fp64 top-two gap is below 4 x the model's worst logit error: the only rows the arg-max comparison leaves out."""
    a = analysis(case)
    return a.gap < 4.0 * a.logit_err[kind]


# ------------------------------------------------------------------------------------------ device side
def tune_fold(v):
    check(lib.rmcl_tune_set(5, v))


class Buffers:
    """dq, rows_out, loss_sum and the workspace at their prescribed sizes between guard bytes, NaN-filled; q, k, queue with copies."""
    BACK = 1 << 16

    def __init__(self, case, B=None, Kq=None):
        B, Kq = case.B if B is None else B, case.Kq if Kq is None else Kq
        q, k, queue, _ = inputs(case)
        self.q, self.k, self.queue = q.to(DEV), k.to(DEV), queue.to(DEV)
        self.keep = (self.q.clone(), self.k.clone(), self.queue.clone())
        nan = float("nan")
        self.ws_bytes = int(lib.rmcl_infonce_ws_bytes(max(B, 1), I64(max(Kq, 128))))
        self.g = {"dq": Guarded(max(B, 1) * PD, torch.float32, self.BACK, nan), "rows": Guarded(max(B, 1) * 10, torch.float32, self.BACK, nan),
                  "lsum": Guarded(1, torch.float32, self.BACK, C0), "ws": Guarded(self.ws_bytes // 4, torch.float32, self.BACK, nan)}

    def refill(self):
        for n in ("dq", "rows", "ws"):
            self.g[n].t.fill_(float("nan"))

    def call(self, entry, with_metrics, B, Kq, T, proj=PD, dq=True, lsum=True, null=()):
        t = {n: (None if n in null else g.t) for n, g in self.g.items()}
        args = [P(None if "q" in null else self.q), P(self.k), P(self.queue), B, proj, I64(Kq), F(T), F(1.0 / (3.0 * max(B, 1))),
                P(t["dq"] if dq else None), P(t["rows"]), P(t["lsum"] if lsum else None), P(t["ws"])]
        if entry == "f32":
            rc = lib.rmcl_infonce_f32(*args, stream())
        else:
            rc = lib.rmcl_infonce_split_bf16(*args, with_metrics, stream())
        torch.cuda.synchronize()
        for n, g in self.g.items():
            assert g.intact(), f"{n}: guard bytes overwritten"
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip((self.q, self.k, self.queue), self.keep)), "an input was written"
        return rc

    def results(self, B, dq=True):
        rows = self.g["rows"].t.view(-1, 10)[:B].cpu()
        assert not bool(torch.isnan(rows).any()), "rows_out holds NaN"
        got = {"loss_i": rows[:, 0], "pred": rows[:, 1].long(), "l_pos": rows[:, 2], "lse": rows[:, 9], "rows": rows}
        got.update({n: rows[:, 3 + j] for j, n in enumerate(METRICS)})
        if dq:
            got["dq"] = self.g["dq"].t.view(-1, PD)[:B].cpu()
            assert not bool(torch.isnan(got["dq"]).any()), "dq holds NaN"
        return got


def loss_sum_bound(case, allowed):
    a = analysis(case)
    return 4 * 2.0 ** -24 * max(C0, float(a.ref["loss_i"].abs().max())) + allowed["loss_i"] * float(a.S.max())


def run_arm(case, arm):
    """Three calls (full; loss_sum = NULL; dq = NULL) with the contract of the docstring; returns the first call's results."""
    entry, wm, key5, kernels, _ = ARMS[arm]
    assert launched(entry, wm, key5, case.Kq)[:2] == kernels, f"{case} does not reach {arm}"
    a = analysis(case)
    allowed = allowed_figures(case, arm)
    mean = float(a.ref["loss_i"].mean())
    buf = Buffers(case)
    try:
        tune_fold(key5)
        check(buf.call(entry, wm, case.B, case.Kq, case.T), "infonce")
        got = buf.results(case.B)
        got["loss_sum"] = float(buf.g["lsum"].t)
        buf.refill()
        check(buf.call(entry, wm, case.B, case.Kq, case.T, lsum=False), "infonce")
        again = buf.results(case.B)
        assert torch.equal(bits(again["rows"]), bits(got["rows"])) and torch.equal(bits(again["dq"]), bits(got["dq"])), "run-to-run difference"
        assert float(buf.g["lsum"].t) == got["loss_sum"], "loss_sum = NULL was written somewhere"
        buf.refill()
        check(buf.call(entry, wm, case.B, case.Kq, case.T, dq=False), "infonce")
        nodq = buf.results(case.B, dq=False)
        assert torch.equal(bits(nodq["rows"]), bits(got["rows"])), "rows_out differs with dq = NULL"
        assert bool(torch.isnan(buf.g["dq"].t).all()), "dq = NULL, yet the dq buffer was written"
        twice = float(buf.g["lsum"].t)
    finally:
        tune_fold(1)
    tol = loss_sum_bound(case, allowed)
    print(f"{case_id(case)} {arm} loss_sum: {got['loss_sum']:.8f} then {twice:.8f} (c0 {C0} + mean {mean:.8f}, tol {tol:.3e})")
    assert abs(got["loss_sum"] - (C0 + mean)) <= tol, "loss_sum after the first call"
    assert abs(twice - (C0 + 2 * mean)) <= 2 * tol, "loss_sum is not +="
    return got


def assert_parity(case, arm, got):
    a = analysis(case)
    kind = model_kind(arm, case.Kq)
    allowed = allowed_figures(case, arm)
    fig = figures(got, a.ref, a.S)
    rec, bad = {}, []
    for n in OUTS if ARMS[arm][1] else OUTS[:-3]:              # (with_metrics = 0: rows_out[:, 6:9] is held to exactly 0 below)
        rec[n] = [float(f"{v:.4g}") for v in (fig[n], a.fig[kind][n], allowed[n], fig[n] / allowed[n] if allowed[n] else float(fig[n] > 0) * 1e30)]
        print(f"{case_id(case)} {arm} [{kind}] {n}: worst row {fig[n]:.3e} (model {a.fig[kind][n]:.3e}, allowed {allowed[n]:.3e})")
        if not fig[n] <= allowed[n]:
            bad.append((n, fig[n], allowed[n]))
    rec["dq_global"] = [float(f"{fig['dq_global']:.4g}"), float(f"{a.fig[kind]['dq_global']:.4g}")]
    PARITY.setdefault(case_id(case), {})[arm] = rec
    if not ARMS[arm][1]:
        assert bool((got["rows"][:, 6:9] == 0).all()), "with_metrics = 0: rows_out[:, 6:9] is not exactly 0"
    info = inputs(case)[3]
    near = near_ties(case, kind)
    assert int(near.sum()) == len(info["dups"]) and all(bool(near[r]) for r in info["dups"]), (near.nonzero().flatten().tolist(), info["dups"])
    wrong = ((got["pred"] != a.argmax) & ~near).nonzero().flatten().tolist()
    assert not wrong, [(r, int(got["pred"][r]), int(a.argmax[r])) for r in wrong[:8]]
    for r, want in info["winners"].items():
        assert int(got["pred"][r]) == want, (r, int(got["pred"][r]), want)
    if BASE[case.family] == "trained" and not info["dups"]:
        assert bool((got["pred"] == 0).all())
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 1. every arm at its shapes and families
@pytest.mark.parametrize("arm,case", ALL, ids=case_id)
def test_arm_matches_fp64_row_by_row(arm, case):
    assert_parity(case, arm, run_arm(case, arm))


# ------------------------------------------------------------------------------------------ 2. the fallback is the exact-f32 kernel
@pytest.mark.parametrize("B,Kq", [(65, 384), (4, 128)])
def test_split_entry_at_odd_kq_gives_the_f32_entry_bits(B, Kq):
    """rmcl_infonce_split_bf16 at Kq % 256 == 128 runs the kernels of rmcl_infonce_f32: the same bits, but for the metrics it zeroes."""
    case = Case("spikes", B, Kq, 0.07)
    f32, m1, m0 = (run_arm(case, arm) for arm in ("f32_odd", "split_fallback_m1", "split_fallback_m0"))
    assert torch.equal(bits(f32["rows"]), bits(m1["rows"])) and torch.equal(bits(f32["dq"]), bits(m1["dq"]))
    keep = [0, 1, 2, 3, 4, 5, 9]
    assert torch.equal(bits(f32["rows"][:, keep]), bits(m0["rows"][:, keep])) and torch.equal(bits(f32["dq"]), bits(m0["dq"]))


@pytest.mark.parametrize("metrics", [1, 0])
def test_split_entry_under_key5_0_is_the_round1_f32_kernel(metrics):
    case = Case("ties", 65, 512, 0.07)
    buf = Buffers(case)
    out = []
    try:
        tune_fold(0)
        for entry in ("f32", "split"):
            buf.refill()
            check(buf.call(entry, metrics, case.B, case.Kq, case.T), "infonce")
            out.append(buf.results(case.B))
    finally:
        tune_fold(1)
    keep = list(range(10)) if metrics else [0, 1, 2, 3, 4, 5, 9]
    assert torch.equal(bits(out[0]["rows"][:, keep]), bits(out[1]["rows"][:, keep])) and torch.equal(bits(out[0]["dq"]), bits(out[1]["dq"]))
    if not metrics:
        assert bool((out[1]["rows"][:, 6:9] == 0).all())
    assert_parity(case, "f32_round1", out[0])


# ------------------------------------------------------------------------------------------ 3. rejections
REJECT = {"proj_64": dict(proj=64), "proj_256": dict(proj=256), "kq_200": dict(Kq=200), "kq_0": dict(Kq=0), "kq_negative": dict(Kq=-128),
          "b_0": dict(B=0), "null_q": dict(null=("q",)), "null_rows": dict(null=("rows",)), "null_ws": dict(null=("ws",))}


@pytest.mark.parametrize("entry", ["f32", "split"])
@pytest.mark.parametrize("what", list(REJECT))
def test_rejected_before_anything_is_written(what, entry):
    """Each returns an error naming infonce and launches nothing: every buffer, NaN-filled rows_out included, keeps its bytes."""
    case = Case("randn", 4, 256, 0.07)
    kw = dict(REJECT[what])
    buf = Buffers(case)
    before = {n: g.raw.clone() for n, g in buf.g.items()}
    rc = buf.call(entry, 1, kw.pop("B", case.B), kw.pop("Kq", case.Kq), case.T, **kw)
    assert rc != 0
    assert b"infonce" in (lib.rmcl_last_error() or b""), lib.rmcl_last_error()
    for n, g in buf.g.items():
        assert torch.equal(g.raw, before[n]), f"{n} was written by a rejected call"
