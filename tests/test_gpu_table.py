"""The table-driven heterogeneous launch (dpm_launch_opts.table_mode, stage_kernel_table / stage_kernel_table_unipc) on the
MI355X.  Kernel level, through the C ABI and between guards (tests/guarded.py): calls of 17, 33 and 200 requests of one n --
the sizes around a tile and a super-tile edge, the largest with several super-tiles per request -- go DPM_TABLE_FILL into a
host tensor, `copy_` to the device, DPM_TABLE_LAUNCH, and must give every request the bits of the numpy double AND of its own
dpm_stage_launch; the launches are counted by kernel name.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import guarded as G
import test_gpu_edges as E
from dpm_solver_amd import _lib as L
from test_gpu_edges import PAIRS, PAIR_IDS
from test_gpu_pool_shapes import MIXES, requests
from test_gpu_unipc_pool import _stage_kernels

gpu = pytest.mark.gpu
DEV = "cuda:0"
CELLS = [(c, n) for c in (17, 33) for n in (8, 2040, 2048, 2056, 4104, 16384)] + [(200, 8), (200, 2056)]
TABLE_MIXES = ("het2", "het3", "unipc")
# mix x guidance x prologue (noise: compile-time, v: generic), the mix innermost
COMBOS = [(mix, g, m) for g in ("uncond", "classifier-free") for m in ("noise", "v") for mix in TABLE_MIXES]
TABLE_GUARD = 4096                                              # bytes on either side of the device table


def combo_of(p, ci):
    """the combo of dtype pair p at CELLS[ci]: 14 consecutive slots per pair cover all 12"""
    return COMBOS[(p * len(CELLS) + ci) % len(COMBOS)]


def test_rotation_covers_every_mix_guidance_and_prologue_per_dtype_pair():
    assert len(COMBOS) == 12 and len(PAIRS) == 5 and all(m in MIXES for m in TABLE_MIXES)
    for p in range(len(PAIRS)):
        assert {combo_of(p, ci) for ci in range(len(CELLS))} == set(COMBOS)
    for count in (17, 33, 200):                                 # every request count meets every mix
        assert {combo_of(p, ci)[0] for p in range(len(PAIRS)) for ci, c in enumerate(CELLS) if c[0] == count} == set(TABLE_MIXES)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class TableCall:
    """the arrays of one per-request-stage call on guarded GPU operands, and its table: a host tensor and a guarded device one.
    `flags` (DPM_TABLE_NOISE / DPM_TABLE_THRESH / DPM_TABLE_BLEND) is the section layout -- the table is sized for the record
    sections those flags put behind the rows -- and the flag word tick() puts on both of its calls"""

    def __init__(self, devs, flags=0):
        self.devs, self.R, self.flags = devs, len(devs), flags
        self.st = (L.Stage * self.R)(*[d.st for d in devs])
        self.bs = (L.Buffers * self.R)(*[d.b for d in devs])
        self.opts = devs[0].opts
        self.ws0 = devs[0].b.workspace                          # request 0's own workspace: what a mode-0 call hands it
        nbytes = L.table_bytes(self.R, flags)
        self.host = torch.full((nbytes,), 0x5A, dtype=torch.uint8)
        self.arena = torch.full((nbytes + 2 * TABLE_GUARD,), 0xC3, dtype=torch.uint8, device=DEV)
        self.dev = self.arena[TABLE_GUARD:TABLE_GUARD + nbytes]
        assert self.host.data_ptr() % 16 == 0 and self.dev.data_ptr() % 16 == 0

    def call(self, mode, table=None):
        self.opts.table_mode = mode
        self.bs[0].workspace = self.ws0 if table is None else table.data_ptr()
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, _stream())
        self.opts.table_mode = 0
        assert rc == 0, (rc, L.lib.dpm_last_error())

    def tick(self, flags=None):
        """FILL into the host tensor, one copy to the device, LAUNCH; both calls with `flags` (default: the layout's)"""
        flags = self.flags if flags is None else flags
        self.call(L.TABLE_FILL | flags, self.host)
        self.dev.copy_(self.host, non_blocking=True)
        self.call(L.TABLE_LAUNCH | flags, self.dev)
        torch.cuda.synchronize()

    def mode0(self):
        self.call(0)
        torch.cuda.synchronize()

    def table_intact(self):
        a = self.arena.cpu()
        n = self.host.numel()
        return bool((a[:TABLE_GUARD] == 0xC3).all() and (a[TABLE_GUARD + n:] == 0xC3).all()
                    and torch.equal(a[TABLE_GUARD:TABLE_GUARD + n], self.host))


def check_table_call(cases, what):
    """one FILL / copy / LAUNCH tick on guarded operands: guards, inputs and bits against the double (verify), the table and its
    guards as the host wrote them, then every request's own dpm_stage_launch into the same, refilled, output arenas: the same
    bits"""
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = TableCall(devs)
    t.tick()
    G.verify_all(devs, wants)
    assert t.table_intact(), (what, "the kernel may only read its table")
    for r, d in enumerate(devs):
        fused = {k: d.arenas[k].raw.clone() for k in G.OUTPUTS}
        for k in G.OUTPUTS:
            d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])
        rc = L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
        for k in G.OUTPUTS:
            assert torch.equal(fused[k], d.arenas[k].raw), (what, r, d.n, k, "differs from the request's own dpm_stage_launch")
    return t


@gpu
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=["%dreq-n%d" % c for c in CELLS])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_table_calls_equal_the_single_launches_and_the_double(p, ci):
    sd, ed = PAIRS[p]
    count, n = CELLS[ci]
    mix, guidance, model = combo_of(p, ci)
    cases = requests(mix, guidance, model, count, sd, ed, seed=7 * p + ci, sizes=[n] * count)
    t = check_table_call(cases, (mix, guidance, model, count, n))
    header = t.host[:16].view(torch.int32).tolist()
    assert header == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1], header


def _table_call(mix, count, sdt, n=2056, **kw):
    return TableCall([c.on(DEV) for c in requests(mix, "uncond", "noise", count, sdt, sdt, sizes=[n] * count, **kw)])


def _names(fn):
    fn()                                                        # (first-launch costs outside the profile)
    return _stage_kernels(fn)


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("mix,family", [("het2", "stage_kernel_table<"), ("het3", "stage_kernel_table<"),
                                        ("unipc", "stage_kernel_table_unipc")])
def test_a_group_of_more_than_16_is_one_table_launch(sdt, mix, family):
    """kernels counted, not bits: 17 and 200 requests under DPM_TABLE_LAUNCH are ONE launch of the table family; the same
    arrays in mode 0 are 2 and 13 launches -- one stage_kernel_het launch per 16 requests, and the 17th request's own"""
    het = "stage_kernel_het_unipc" if mix == "unipc" else "stage_kernel_het<"
    for count, launches, het_launches in ((17, 2, 1), (200, 13, 13)):
        t = _table_call(mix, count, sdt)
        names = _names(t.tick)
        assert len(names) == 1 and family in names[0], (count, names)
        names = _names(t.mode0)
        assert len(names) == launches and sum(het in n for n in names) == het_launches, (count, names)
        assert not any("stage_kernel_table" in n for n in names), (count, names)


@gpu
def test_16_requests_keep_the_kernarg_launch():
    for mix, het in (("het2", "stage_kernel_het<"), ("unipc", "stage_kernel_het_unipc")):
        t = _table_call(mix, 16, torch.float16)
        names = _names(t.tick)
        assert len(names) == 1 and het in names[0] and "stage_kernel_table" not in names[0], names
        assert t.host[:16].view(torch.int32).tolist()[2:] == [16, 0]


@gpu
@pytest.mark.parametrize("mix", ["het2", "unipc"])
def test_a_member_the_fused_family_does_not_take_gets_its_own_launch_in_the_same_call(mix):
    """the middle member's n is no multiple of 8: its own launch, the other 20 their table launch, in one call, right bits"""
    sdt = torch.float16
    sizes = [2056] * 10 + [2059] + [2056] * 10
    for guidance in ("uncond", "classifier-free"):
        cases = requests(mix, guidance, "noise", len(sizes), sdt, sdt, sizes=sizes, seed=5)
        t = check_table_call(cases, ("fall back", mix, guidance))
        assert t.host[:16].view(torch.int32).tolist()[2:] == [21, 1]
        names = _names(t.tick)
        assert len(names) == 2 and sum("stage_kernel_table" in n for n in names) == 1, names
