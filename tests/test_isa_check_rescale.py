"""build()'s ISA check (__graft_entry__.scan_disassembly) on synthetic disassembly of unit E: the guidance-rescale kernels -- the
lone stage_rescale_kernel and the table's stage_rescale_kernel_table, which hold a sample's outputs in up to 233 of 256
registers -- are under the no-scratch rule, and do not count against MAX_STAGE_KERNELS (their own name, their own budget)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

LONE = "_ZN12_GLOBAL__N_120stage_rescale_kernelIffEEvPKT_S3_PKT0_S6_S3_S3_PS1_S7_S7_lNS_7KParamsEi"
TABLE = "_ZN12_GLOBAL__N_126stage_rescale_kernel_tableIffEEvPKNS_8TableRowElj"
GOOD = """
0000000000001000 <%s>:
	global_load_dwordx4 v[4:7], v[2:3], off nt
	global_store_dwordx4 v[10:11], v[0:3], off
0000000000002000 <%s>:
	s_load_dwordx4 s[8:11], s[4:5], 0x0
	global_load_dwordx4 v[4:7], v[2:3], off nt
	global_store_dwordx4 v[10:11], v[4:7], off sc0 sc1
	s_nop 1
""".strip("\n").splitlines()
GOOD = [GOOD[0] % LONE] + GOOD[1:3] + [GOOD[3] % TABLE] + GOOD[4:]


def test_accepts_the_listing_without_scratch():
    n_wt, n_kernels, spilled = G.scan_disassembly(GOOD)
    assert (n_wt, n_kernels) == (1, 0) and not spilled


@pytest.mark.parametrize("name", [LONE, TABLE], ids=["lone", "table"])
@pytest.mark.parametrize("ins", ["scratch_load_dword v1, off, s32", "scratch_store_dword off, v40, s32 offset:4"])
def test_rejects_scratch_in_a_rescale_kernel(name, ins):
    i = next(i for i, ln in enumerate(GOOD) if "<%s>" % name in ln)
    bad = GOOD[:i + 2] + ["\t" + ins] + GOOD[i + 2:]
    with pytest.raises(AssertionError, match="stage_rescale_kernel.*spills to scratch"):
        G.scan_disassembly(bad)
    G.scan_disassembly(GOOD[:i + 2] + ["\tv_mov_b32 v1, v2"] + GOOD[i + 2:])      # the same listing without it


def test_scratch_outside_the_stage_kernels_is_not_this_rule():
    other = ["0000000000003000 <_ZN12_GLOBAL__N_116add_noise_kernelIfLb1EEEvPKT_>:", "\tscratch_load_dword v1, off, s32"]
    G.scan_disassembly(GOOD + other)
