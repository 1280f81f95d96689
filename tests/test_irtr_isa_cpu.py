"""CPU (hipcc cross-compiles gfx950 without a GPU): the image-text retrieval kernels of csrc/irtr.hip - score, cross-entropy, backward,
the visual_embed assembly and the rank-pass assembly - use no scratch memory and spill no registers (the same reading of the compiler's
assembly as tests/test_nlvr2_isa_cpu.py)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]
KERNELS = ("irtr_score_kernel", "irtr_ce_kernel", "irtr_bwd_kernel", "visual_assemble_kernel", "rank_assemble_kernel")


def test_irtr_kernels_use_no_scratch_and_do_not_spill():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "irtr.s")
        r = subprocess.run(["hipcc", *FLAGS, os.path.join(CSRC, "irtr.hip"), "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        isa = open(dst).read()
    sizes = dict(re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa))
    for k in KERNELS:
        mine = [n for n in sizes if k in n]
        assert mine, (k, list(sizes)[:8])
        for n in mine:
            assert int(sizes[n]) == 0, (n, sizes[n])
            for field in ("sgpr_spill_count", "vgpr_spill_count"):
                m = re.search(r"\.name:\s+" + re.escape(n) + r"\b.*?\." + field + r":\s+(\d+)", isa, re.S)
                assert m is not None and int(m.group(1)) == 0, (n, field, m and m.group(1))
    assert "atomic" not in "".join(l for l in isa.splitlines() if not l.lstrip().startswith((";", ".", "//"))).lower()
