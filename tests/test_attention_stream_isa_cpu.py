"""CPU (hipcc cross-compiles gfx950 without a GPU): no kernel of csrc/attention_stream.hip uses scratch memory.

The streaming attention kernels keep an online-softmax state, a 64-key score block and the output accumulators in registers; a spill
would put private-segment traffic into the key loop.  Compiled with the flags of tests/test_isa_budget_cpu.py; a resource check only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.test_isa_budget_cpu import CSRC, FLAGS


def test_no_streaming_attention_kernel_uses_scratch():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "attention_stream.s")
        r = subprocess.run(["hipcc", *FLAGS, os.path.join(CSRC, "attention_stream.hip"), "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(dst).read()
    sizes = re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", text)
    names = " ".join(n for n, _ in sizes)
    assert all(k in names for k in ("attn_stream_fwd_kernel", "attn_stream_dq_kernel", "attn_stream_dkv_kernel")), names
    assert not [(n[:80], int(s)) for n, s in sizes if int(s) != 0]
