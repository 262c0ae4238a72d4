"""Mask-blend stages in the table-driven launch (DPM_TABLE_BLEND, stage_kernel_table_blend) on the MI355X.  Kernel level, through
the C ABI and between guards (tests/guarded.py), as tests/test_gpu_table.py / test_gpu_table_sde.py: calls of 1, 2, 17, 33 and
200 DPM_F_BLEND requests of one n -- the sizes around a tile and a super-tile edge -- go DPM_TABLE_FILL | DPM_TABLE_BLEND into a
host tensor, `copy_` to a guarded device table, DPM_TABLE_LAUNCH | DPM_TABLE_BLEND, and must give every request the bits of the
numpy double AND of its own dpm_stage_launch with the same blend.  Within a launch the rows rotate the three forms (each with
coefficients of its own), STORE_M, a named or null x_out2 under guidance, a null or non-null blend_b, and the mask periods n,
n/4 (where that is whole 8-element groups) and 8 -- so one launch holds rows that take the split tile layout (4-byte states,
a period of whole 2048-element tiles) and rows that cannot.  The launches are counted by kernel name.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import guarded as G
import test_gpu_edges as E
from dpm_solver_amd import _lib as L
from test_gpu_edges import PAIRS, PAIR_IDS
from test_gpu_pool_shapes import requests
from test_gpu_table import TABLE_GUARD, TableCall
from test_gpu_unipc_pool import _stage_kernels

gpu = pytest.mark.gpu
DEV = "cuda:0"
CELLS = [(c, n) for c in (1, 2, 17, 33) for n in (8, 2040, 2048, 2056, 4104, 16384)] + [(200, 8), (200, 2056)]
COMBOS = [(g, m) for g in ("uncond", "classifier-free") for m in ("noise", "v")]      # guidance x prologue (v: generic)
FORMS = ("LIN1", "TWO", "MS3")
BLEND = L.TABLE_BLEND


def combo_of(p, ci):
    return COMBOS[(p + ci) % len(COMBOS)]


def periods_of(n):
    return (n, n // 4 if (n // 4) % 8 == 0 else 8, 8)


def blend_requests(count, n, guidance, model, sd, ed, seed):
    """the CPU cases of one call: request r takes FORMS[r % 3], STORE_M for r % 2 == 0, x_out2 (guidance only) unless
    r % 4 == 3, a null blend_b for r % 5 == 4 and the period periods_of(n)[(r // 3) % 3]; coefficients of its own"""
    out = []
    for r in range(count):
        st = E.make_stage(FORMS[r % 3], guidance, model, store_m=(r % 2 == 0), blend=True, seed=seed * 131 + r)
        out.append(G.GuardedLaunch("table-blend", st, n, sd, ed, dup=(guidance != "uncond" and r % 4 != 3),
                                   blend=(periods_of(n)[(r // 3) % 3], r % 5 != 4), seed=seed, req=r, per_request_stages=True))
    return out


def test_rotation_covers_guidance_prologue_forms_periods_and_layouts():
    for p in range(len(PAIRS)):
        assert {combo_of(p, ci) for ci in range(len(CELLS))} == set(COMBOS)
    for count in (1, 2, 17, 33):
        assert {combo_of(p, ci) for p in range(len(PAIRS)) for ci, c in enumerate(CELLS) if c[0] == count} == set(COMBOS)
    for count in (17, 33, 200):                                  # within ONE launch
        rows = [(FORMS[r % 3], r % 2 == 0, r % 4 != 3, r % 5 != 4, (r // 3) % 3) for r in range(count)]
        assert {(f, k) for f, _, _, _, k in rows} == {(f, k) for f in FORMS for k in range(3)}
        for i in (1, 2, 3):
            assert {row[i] for row in rows} == {True, False}
    # periods of whole tiles (the split layout of a 4-byte state) next to a period of 8 (never split) where n has whole tiles
    assert periods_of(16384) == (16384, 4096, 8) and periods_of(2048) == (2048, 512, 8) and periods_of(2056) == (2056, 8, 8)
    assert all(k % 8 == 0 and n % k == 0 for _, n in CELLS for k in periods_of(n))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class BlendTableCall(TableCall):
    """TableCall with the record sections behind the rows (`noise`: the noise section in front of the blend section)"""

    def __init__(self, devs, noise=False):
        super().__init__(devs)
        self.rec0 = L.TABLE_HEADER_BYTES + self.R * (L.TABLE_ROW_BYTES + (L.TABLE_NOISE_BYTES if noise else 0))
        nbytes = self.rec0 + self.R * L.TABLE_BLEND_BYTES
        self.host = torch.full((nbytes,), 0x5A, dtype=torch.uint8)
        self.arena = torch.full((nbytes + 2 * TABLE_GUARD,), 0xC3, dtype=torch.uint8, device=DEV)
        self.dev = self.arena[TABLE_GUARD:TABLE_GUARD + nbytes]
        assert self.host.data_ptr() % 16 == 0 and self.dev.data_ptr() % 16 == 0

    def tick(self, flag=BLEND):
        self.call(L.TABLE_FILL | flag, self.host)
        self.dev.copy_(self.host, non_blocking=True)
        self.call(L.TABLE_LAUNCH | flag, self.dev)
        torch.cuda.synchronize()

    def records(self, count):
        return self.host[self.rec0:self.rec0 + count * L.TABLE_BLEND_BYTES].view(torch.int64).reshape(count, 6)


def _refill(d):
    for k in G.OUTPUTS:
        d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])


@gpu
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=["%dreq-n%d" % c for c in CELLS])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_table_blend_calls_equal_the_single_launches_and_the_double(p, ci):
    sd, ed = PAIRS[p]
    count, n = CELLS[ci]
    guidance, model = combo_of(p, ci)
    cases = blend_requests(count, n, guidance, model, sd, ed, seed=7 * p + ci)
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = BlendTableCall(devs)
    t.tick()
    G.verify_all(devs, wants)
    assert t.table_intact(), "the kernel may only read its table"
    assert t.host[:16].view(torch.int32).tolist() == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1]
    rec = t.records(count)
    assert rec[:, 0].tolist() == [d.b.mask for d in devs] and rec[:, 1].tolist() == [d.b.blend_a for d in devs]
    assert rec[:, 2].tolist() == [d.b.blend_b or 0 for d in devs] and rec[:, 3].tolist() == [d.b.mask_period for d in devs]
    for r, d in enumerate(devs):                                  # ... and the bits of every request's own dpm_stage_launch
        fused = {k: d.arenas[k].raw.clone() for k in G.OUTPUTS}
        _refill(d)
        rc = L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
        for k in G.OUTPUTS:
            assert torch.equal(fused[k], d.arenas[k].raw), (r, n, k, "differs from the request's own dpm_stage_launch")


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_without_the_flag_the_blend_section_is_neither_written_nor_read(sdt):
    """the same arrays under table_mode 1 / 2: every request is its own launch (version 210), right bits, and the record
    section keeps the bytes it had on the host and on the device"""
    cases = blend_requests(17, 2056, "uncond", "noise", sdt, sdt, seed=3)
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = BlendTableCall(devs)
    names = _stage_kernels(lambda: t.tick(0))
    G.verify_all(devs, wants)
    assert t.table_intact()
    assert t.host[:16].view(torch.int32).tolist()[2:] == [17, 0] and bool((t.host[16:] == 0x5A).all())
    assert len(names) == 17 and not any("stage_kernel_table" in n for n in names), names


def _names(fn):
    fn()                                                        # (first-launch costs outside the profile)
    return _stage_kernels(fn)


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_blend_groups_are_one_table_blend_launch(sdt):
    for count in (1, 17, 200):
        devs = [c.on(DEV) for c in blend_requests(count, 2056, "uncond", "noise", sdt, sdt, seed=count)]
        t = BlendTableCall(devs)
        names = _names(t.tick)
        assert len(names) == 1 and "stage_kernel_table_blend" in names[0], (count, names)


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_plain_sde_and_blend_groups_each_get_their_kernel(sdt):
    """one call, DPM_TABLE_NOISE | DPM_TABLE_BLEND: 20 plain requests, 5 SDE requests, 19 blend requests and one DENOISE stage
    with a blend -- three runs of rows, three table kernels of three families, and the DENOISE request's own launch; every
    request with the bits of the double"""
    import sde_double as SD
    n = 2056
    cache, old = {}, SD.Z_SOURCE[0]

    def z(seed, index, m):
        if (seed, index) not in cache:
            cache[(seed, index)] = E.kernel_z(seed, index, n)
        return cache[(seed, index)][:m]
    SD.Z_SOURCE[0] = z
    try:
        plain = requests("het3", "uncond", "noise", 20, sdt, sdt, seed=1, sizes=[n] * 20)
        sde = requests("noise", "uncond", "noise", 5, sdt, sdt, seed=2, sizes=[n] * 5)
        blend = blend_requests(19, n, "uncond", "noise", sdt, sdt, seed=3)
        last = G.GuardedLaunch("table-blend", E.make_stage("DENOISE", blend=True, seed=9), n, sdt, sdt, blend=(8, True), seed=4,
                               per_request_stages=True)
        cases = [plain[0], sde[0], blend[0]] + plain[1:] + [last] + sde[1:] + blend[1:]
        wants = [G.run_double(c) for c in cases]
    finally:
        SD.Z_SOURCE[0] = old
    devs = [c.on(DEV) for c in cases]
    t = BlendTableCall(devs, noise=True)
    flag = L.TABLE_NOISE | BLEND
    t.tick(flag)
    G.verify_all(devs, wants)
    assert t.table_intact()
    assert t.host[:16].view(torch.int32).tolist()[2:] == [45, 3]
    for d in devs:
        _refill(d)
    names = _stage_kernels(lambda: t.tick(flag))
    G.verify_all(devs, wants)
    assert len(names) == 4, names
    assert sum("stage_kernel_table_blend" in k for k in names) == 1 and sum("stage_kernel_table_noise" in k for k in names) == 1
    assert sum("stage_kernel_table<" in k or "stage_kernel_tableI" in k for k in names) == 1, names
