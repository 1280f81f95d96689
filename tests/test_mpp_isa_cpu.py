"""CPU (hipcc cross-compiles gfx950 without a GPU): the masked-patch-prediction kernels of csrc/mpp.hip and the mask-token substitution
kernels of csrc/embed_misc.hip use no scratch memory (the gather / scatter and the transform kernels are csrc/head_transform.hip's:
tests/test_head_transform_isa_cpu.py) - the same reading of the compiler's assembly as tests/test_nlvr2_isa_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]


def _isa(name):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, name + ".s")
        r = subprocess.run(["hipcc", *FLAGS, os.path.join(CSRC, name), "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(dst).read()


@pytest.mark.parametrize("src,kernels", [("mpp.hip", ("mpp_labels_kernel", "mpp_compact_kernel", "mpp_ce_fwd_kernel", "mpp_stats_kernel",
                                                      "mpp_ce_bwd_kernelItE", "mpp_ce_bwd_kernelIfE", "mpp_dbias_part_kernelItE", "mpp_dbias_part_kernelIfE", "mpp_dbias_merge_kernel",
                                                      "mpp_logits_copy_kernel")),
                                         ("embed_misc.hip", ("mask_token_fwd_kernel", "mask_token_bwd_kernelIfE", "mask_token_bwd_kernelItE", "mask_token_merge_kernel"))])
def test_mpp_kernels_use_no_scratch(src, kernels):
    isa = _isa(src)
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa)
    names = " ".join(n for n, _ in sizes)
    for k in kernels:
        assert k in names, (k, names[:400])
    spilled = [(n[:80], int(s)) for n, s in sizes if int(s) != 0 and ("mpp_" in n or "mask_token" in n)]
    assert not spilled, spilled
