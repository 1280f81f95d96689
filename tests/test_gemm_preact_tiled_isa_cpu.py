"""CPU (hipcc cross-compiles gfx950 without a GPU): what the tiled pre-activation stash (gemm.h EPI_PREACT_TILED) removes from the
192x384 kernel, read from the compiler's own assembly.  Every comparison is between instantiations of ONE compile of gemm_sw.hip -
no absolute numbers:
  * the tiled fc2-dX form is scratch-free, stages nothing but its operands by LDS-DMA (no more such instructions than the plain fc1
    form without a stash) and runs fewer VALU instructions and fewer barriers behind its last MFMA than the row-major form, whose
    GELU' operand comes through LDS;
  * the tiled fc1-with-stash form is scratch-free and writes less to LDS behind its last MFMA than the row-major stash form."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]

# gemm_sw_kernel<B_KC = true, AUX, TO = bf16 (t), LNF, DROP = false>: AUX 0 none / row-major stash, 2 GELU' through LDS, 3 GELU' from the tiled stash, 4 tiled stash
FC1, FC1_FOLDED, FC2DX, FC2DX_TILED, FC1_TILED, FC1_FOLDED_TILED = "Li0EtLi0E", "Li0EtLi1E", "Li2EtLi0E", "Li3EtLi0E", "Li4EtLi0E", "Li4EtLi1E"


@pytest.fixture(scope="module")
def kernels():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "gemm_sw.s")
        r = subprocess.run(["hipcc", *FLAGS, os.path.join(CSRC, "gemm_sw.hip"), "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(dst).read()
    out = {}
    lines = text.split("\n")
    for key in (FC1, FC1_FOLDED, FC2DX, FC2DX_TILED, FC1_TILED, FC1_FOLDED_TILED):
        name = f"_Z14gemm_sw_kernelILb1E{key}Lb0EEv8GemmArgsiii"
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        body = []
        for l in lines[start + 1:]:
            if l.strip().startswith(".Lfunc_end"):
                break
            body.append(l.strip())
        last = max(i for i, l in enumerate(body) if l.startswith("v_mfma"))
        scratch = int(re.search(r"\.set " + re.escape(name) + r"\.private_seg_size, (\d+)", text).group(1))
        out[key] = {"body": body, "tail": body[last:], "scratch": scratch}
    return out


def count(lines, prefix):
    return sum(1 for l in lines if l.startswith(prefix))


def test_tiled_fc2dx_sheds_the_aux_path(kernels):
    new, old, plain = kernels[FC2DX_TILED], kernels[FC2DX], kernels[FC1]
    assert new["scratch"] == 0
    assert 0 < count(new["body"], "global_load_lds") <= count(plain["body"], "global_load_lds") < count(old["body"], "global_load_lds")
    assert count(new["tail"], "v_") < count(old["tail"], "v_")
    assert count(new["tail"], "s_barrier") < count(old["tail"], "s_barrier")


@pytest.mark.parametrize("new,old", [(FC1_TILED, FC1), (FC1_FOLDED_TILED, FC1_FOLDED)])
def test_tiled_fc1_keeps_no_stash_image(kernels, new, old):
    assert kernels[new]["scratch"] == 0
    assert 0 < count(kernels[new]["tail"], "ds_write") < count(kernels[old]["tail"], "ds_write")
