"""CPU (hipcc cross-compiles gfx950 without a GPU): every kernel of csrc/head_transform.hip - the prediction-head transform the MLM and
the MPP head share - is present in every instantiation that is launched and uses no scratch memory, and the file's assembly holds no
float atomic and no compare-and-swap loop (every output has one owner and a fixed summation order).  The assertions are those
tests/test_mlm_isa_cpu.py and tests/test_mpp_isa_cpu.py made about these kernels while the two heads each carried a copy."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc", "head_transform.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]
# operand type bf16 ("It": unsigned short) / fp32 ("If"), D = 256 NV ("Li1E" / "Li3E"), with the transposed copy hT (MLM, "Lb1E") or not (MPP)
KERNELS = ("pred_gather_kernel", "pred_scatter_kernel", "pred_param_grad_kernel", "pred_gelu_ln_bwd_kernelILi1E", "pred_gelu_ln_bwd_kernelILi3E",
           "pred_gelu_ln_fwd_kernelItLi1ELb1E", "pred_gelu_ln_fwd_kernelItLi3ELb1E", "pred_gelu_ln_fwd_kernelIfLi1ELb1E", "pred_gelu_ln_fwd_kernelIfLi3ELb1E",
           "pred_gelu_ln_fwd_kernelItLi1ELb0E", "pred_gelu_ln_fwd_kernelItLi3ELb0E", "pred_gelu_ln_fwd_kernelIfLi1ELb0E", "pred_gelu_ln_fwd_kernelIfLi3ELb0E")


@pytest.fixture(scope="module")
def isa():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "head_transform.s")
        r = subprocess.run(["hipcc", *FLAGS, SRC, "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(dst).read()


def test_transform_kernels_are_present_and_use_no_scratch(isa):
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    names = " ".join(n for n, _ in sizes)
    for k in KERNELS:
        assert k in names, k
    spilled = [(n[:80], int(s)) for n, s in sizes if int(s) != 0]
    assert not spilled, spilled


def test_no_float_atomics_in_the_file(isa):
    for word in ("global_atomic_add_f32", "global_atomic_pk_add", "cmpswap", "flat_atomic_add_f32", "ds_add_f32", "ds_add_rtn_f32"):
        assert word not in isa, word
