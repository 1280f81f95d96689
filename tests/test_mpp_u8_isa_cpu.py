"""CPU (hipcc cross-compiles gfx950 without a GPU): the byte-feed label kernel of csrc/mpp.hip (rmcl_mpp_labels_u8) compiles for gfx950
and uses no scratch memory, and its register allocation spills nothing - the same reading of the compiler's assembly as
tests/test_mpp_isa_cpu.py, plus the spill counts of the kernel's metadata record."""
import re

from tests.test_mpp_isa_cpu import _isa


def test_mpp_labels_u8_kernel_uses_no_scratch_and_spills_nothing():
    isa = _isa("mpp.hip")
    sizes = dict(re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", isa))
    mine = [n for n in sizes if "mpp_labels_u8_kernel" in n]
    assert len(mine) == 1, sorted(sizes)[:40]
    assert int(sizes[mine[0]]) == 0, (mine[0], sizes[mine[0]])
    record = re.search(r"\.name:\s+" + re.escape(mine[0]) + r"\n(.*?)\.wavefront_size", isa, re.S)
    assert record is not None
    fields = dict(re.findall(r"\.(private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count):\s+(\d+)", record.group(1)))
    assert fields == {"private_segment_fixed_size": "0", "sgpr_spill_count": "0", "vgpr_spill_count": "0"}, fields
