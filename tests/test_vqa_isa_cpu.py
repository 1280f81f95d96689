"""CPU (hipcc cross-compiles gfx950 without a GPU): no kernel of csrc/vqa.hip uses scratch memory - the same reading of the compiler's
own assembly as tests/test_isa_budget_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc", "vqa.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def isa():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "vqa.s")
        r = subprocess.run(["hipcc", *FLAGS, SRC, "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(dst).read()


def test_vqa_kernels_use_no_scratch(isa):
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    names = " ".join(n for n, _ in sizes)
    for k in ("vqa_ln_gelu_fwd_kernel", "vqa_ln_gelu_bwd_kernel", "vqa_ln_param_grad_kernel", "vqa_bce_row_kernel", "vqa_bce_finish_kernel",
              "vqa_targets_dense_kernel"):
        assert k in names, k
    spilled = [(n[:80], int(s)) for n, s in sizes if int(s) != 0]
    assert not spilled, spilled
