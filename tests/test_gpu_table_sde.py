"""SDE stages in the table-driven launch (DPM_TABLE_NOISE, stage_kernel_table_noise) on the MI355X.  Kernel level, through the C
ABI and between guards (tests/guarded.py), as tests/test_gpu_table.py: calls of 1, 2, 17, 33 and 200 SDE requests of one n -- the
sizes around a tile and a super-tile edge -- go DPM_TABLE_FILL | DPM_TABLE_NOISE into a host tensor, `copy_` to a guarded
device table, DPM_TABLE_LAUNCH | DPM_TABLE_NOISE, and must give every request the bits of the numpy double fed the kernel's own
z AND of its own dpm_stage_launch.  The base of a row's counter (dpm_buffers.noise_sample0): the five samples of one request
as five rows equal the request's single launch bit for bit, and a base beyond 2^32 blocks meets the noise contract's float64
restatement at those block indices.  The launches are counted by kernel name.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as G
import sde_double as SD
import test_gpu_edges as E
from dpm_solver_amd import _lib as L
from test_gpu_edges import PAIRS, PAIR_IDS
from test_gpu_pool_shapes import requests
from test_gpu_table import TABLE_GUARD, TableCall
from test_gpu_unipc_pool import _stage_kernels

gpu = pytest.mark.gpu
DEV = "cuda:0"
CELLS = [(c, n) for c in (1, 2, 17, 33) for n in (8, 2040, 2048, 2056, 4104, 16384)] + [(200, 8), (200, 2056)]
NMAX = 16384
COMBOS = [(g, m) for g in ("uncond", "classifier-free") for m in ("noise", "v")]      # guidance x prologue (v: generic)
FILL_N, LAUNCH_N = L.TABLE_FILL | L.TABLE_NOISE, L.TABLE_LAUNCH | L.TABLE_NOISE


def combo_of(p, ci):
    return COMBOS[(p + ci) % len(COMBOS)]


def test_rotation_covers_guidance_and_prologue_per_dtype_pair_and_request_count():
    for p in range(len(PAIRS)):
        assert {combo_of(p, ci) for ci in range(len(CELLS))} == set(COMBOS)
    for count in (1, 2, 17, 33):
        assert {combo_of(p, ci) for p in range(len(PAIRS)) for ci, c in enumerate(CELLS) if c[0] == count} == set(COMBOS)


@pytest.fixture(scope="module")
def gpu_z():
    """test_gpu_edges.gpu_z at this file's largest n: the doubles take the kernel's own z, one pure-noise dpm_stage_launch of
    NMAX elements per (seed, stage index), cached"""
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    cache, old = {}, SD.Z_SOURCE[0]

    def z(seed, index, n):
        if (seed, index) not in cache:
            cache[(seed, index)] = E.kernel_z(seed, index, NMAX)
        assert n <= NMAX
        return cache[(seed, index)][:n]
    SD.Z_SOURCE[0] = z
    yield z
    SD.Z_SOURCE[0] = old
    torch.cuda.synchronize()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class NoiseTableCall(TableCall):
    """TableCall with the noise section behind the rows and DPM_TABLE_NOISE on both modes; `bufs`: records of its own"""

    def __init__(self, devs, st=None, bs=None):
        super().__init__(devs)
        if st is not None:
            self.st, self.bs, self.R = st, bs, len(bs)
        nbytes = L.TABLE_HEADER_BYTES + self.R * (L.TABLE_ROW_BYTES + L.TABLE_NOISE_BYTES)
        self.host = torch.full((nbytes,), 0x5A, dtype=torch.uint8)
        self.arena = torch.full((nbytes + 2 * TABLE_GUARD,), 0xC3, dtype=torch.uint8, device=DEV)
        self.dev = self.arena[TABLE_GUARD:TABLE_GUARD + nbytes]
        assert self.host.data_ptr() % 16 == 0 and self.dev.data_ptr() % 16 == 0

    def tick(self, flag=L.TABLE_NOISE):
        self.call(L.TABLE_FILL | flag, self.host)
        self.dev.copy_(self.host, non_blocking=True)
        self.call(L.TABLE_LAUNCH | flag, self.dev)
        torch.cuda.synchronize()

    def tick_208(self):
        self.tick(0)

    def records(self):
        o = L.TABLE_HEADER_BYTES + self.R * L.TABLE_ROW_BYTES
        return self.host[o:].view(torch.int32).reshape(self.R, 8)


@gpu
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=["%dreq-n%d" % c for c in CELLS])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_table_noise_calls_equal_the_single_launches_and_the_double(p, ci, gpu_z):
    sd, ed = PAIRS[p]
    count, n = CELLS[ci]
    guidance, model = combo_of(p, ci)
    cases = requests("noise", guidance, model, count, sd, ed, seed=7 * p + ci, sizes=[n] * count)
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = NoiseTableCall(devs)
    t.tick()
    G.verify_all(devs, wants)
    assert t.table_intact(), "the kernel may only read its table"
    assert t.host[:16].view(torch.int32).tolist() == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1]
    rec = t.records()
    assert rec[:, 0].tolist() == [1000 + r for r in range(count)] and rec[:, 2].tolist() == [1 + r % 4 for r in range(count)]
    assert not rec[:, 4:].any()
    for r, d in enumerate(devs):                                  # ... and the bits of every request's own dpm_stage_launch
        fused = {k: d.arenas[k].raw.clone() for k in G.OUTPUTS}
        for k in G.OUTPUTS:
            d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])
        rc = L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
        for k in G.OUTPUTS:
            assert torch.equal(fused[k], d.arenas[k].raw), (r, n, k, "differs from the request's own dpm_stage_launch")


@gpu
@pytest.mark.parametrize("per", [8, 2056])
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_five_rows_with_their_bases_are_the_request_of_five_samples(sdt, per):
    """ONE dpm_stage_launch over a [5, per] noise stage against a flagged table call whose rows 0..4 point at the five samples
    with noise_sample0 = 0..4 (12 more SDE requests pad the group to 17): the same bits in x_out and m_out, guards included"""
    st = E.make_stage(("LIN1", "TWO")[per > 8], noise=True, store_m=True, seed=per)
    case = G.GuardedLaunch("table-noise-base", st, 5 * per, sdt, sdt, batch=5, seed=per, noise_seed=0xFEEDFACE12345678)
    d = case.on(DEV)
    L.check(L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream()))
    torch.cuda.synchronize()
    d.verify()
    single = {k: d.arenas[k].raw.clone() for k in G.OUTPUTS}
    for k in G.OUTPUTS:
        d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])
    pad = [c.on(DEV) for c in requests("noise", "uncond", "noise", 12, sdt, sdt, seed=3, sizes=[per] * 12)]
    d.opts.per_request_stages = 1
    R = 5 + len(pad)
    sts, bs = (L.Stage * R)(*([d.st] * 5 + [q.st for q in pad])), (L.Buffers * R)(*([d.b] * 5 + [q.b for q in pad]))
    es = d.arenas["x"].es
    for k in range(5):
        b = bs[k]
        for f in ("x", "e0", "h1", "x_out", "m_out"):
            if getattr(b, f):
                setattr(b, f, getattr(b, f) + k * per * es)
        b.n, b.batch, b.noise_sample0 = per, 1, k
    t = NoiseTableCall([d] + pad, sts, bs)
    t.tick()
    assert t.table_intact()
    assert t.host[:16].view(torch.int32).tolist()[2:] == [R, 1]
    assert t.records()[:5, 4].tolist() == [k * per // 4 for k in range(5)]
    for k in G.OUTPUTS:
        assert torch.equal(single[k], d.arenas[k].raw), (k, "the five rows differ from the request's own launch")
    d.verify()
    # (sample 1 does not simply repeat sample 0's noise: with base 0 in every row the bits differ)
    for k in range(5):
        bs[k].noise_sample0 = 0
    for k in G.OUTPUTS:
        d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])
    t.tick()
    assert not torch.equal(single["x_out"], d.arenas["x_out"].raw)
    a = d.arenas["x_out"]
    assert torch.equal(single["x_out"][:a.lead + per], a.raw[:a.lead + per])


def _z64_at(seed, index, g0, n):
    """the contract's z in float64 at Philox block indices g0 + arange(n / 4)"""
    g = np.uint64(g0) + np.arange(n // 4, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    r = SD.philox4x32_10((g & m, g >> np.uint64(32), np.full_like(g, index), np.zeros_like(g)), (seed & 0xFFFFFFFF, seed >> 32))
    rad0, rad1 = np.sqrt(-2.0 * np.log(SD.unit(r[0]))), np.sqrt(-2.0 * np.log(SD.unit(r[2])))
    a1, a3 = 2.0 * np.pi * SD.unit(r[1]), 2.0 * np.pi * SD.unit(r[3])
    return np.stack([rad0 * np.cos(a1), rad0 * np.sin(a1), rad1 * np.cos(a3), rad1 * np.sin(a3)], axis=1).reshape(-1)


@gpu
def test_a_base_beyond_2_to_the_32_blocks_reaches_the_high_counter_word():
    n, k, seed, index = 16384, (1 << 21) + 1, 0x0123456789ABCDEF, 5
    g0 = k * n // 4
    assert g0 >= 1 << 32
    assert np.array_equal(_z64_at(seed, index, 0, n), SD.noise_z64(seed, index, n))          # (the restatement, at base 0)
    case = G.GuardedLaunch("table-noise-high", E.noise_stage(index), n, torch.float32, torch.float32, seed=1, noise_seed=seed,
                           per_request_stages=True)
    d = case.on(DEV)
    d.b.noise_sample0 = k
    t = NoiseTableCall([d])
    t.tick()
    d.verify()
    assert t.table_intact() and t.records()[0, 4:6].tolist() == [g0 & 0xFFFFFFFF, g0 >> 32]
    got = d.arenas["x_out"].payload().numpy().astype(np.float64)
    want = _z64_at(seed, index, g0, n)
    assert np.all(np.abs(got - want) <= 1e-5 * np.maximum(1.0, np.abs(want))), float(np.max(np.abs(got - want)))
    assert not np.array_equal(got.astype(np.float32), E.kernel_z(seed, index, n))              # not the z at base 0 ...
    low = _z64_at(seed, index, g0 & 0xFFFFFFFF, n)                                              # ... nor the low word's alone
    assert not np.all(np.abs(got - low) <= 1e-5 * np.maximum(1.0, np.abs(low)))


def _names(fn):
    fn()                                                        # (first-launch costs outside the profile)
    return _stage_kernels(fn)


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_sde_groups_are_one_table_noise_launch(sdt):
    """kernels counted, not bits: 17 and 200 SDE requests under DPM_TABLE_LAUNCH | DPM_TABLE_NOISE are ONE
    stage_kernel_table_noise launch; the same arrays without the flag are version 208's launches -- stage_kernel_het_noise per
    16 requests, and the 17th request's own"""
    for count, launches, het_launches in ((17, 2, 1), (200, 13, 13)):
        devs = [c.on(DEV) for c in requests("noise", "uncond", "noise", count, sdt, sdt, sizes=[2056] * count)]
        t = NoiseTableCall(devs)
        names = _names(t.tick)
        assert len(names) == 1 and "stage_kernel_table_noise" in names[0], (count, names)
        names = _names(t.tick_208)
        assert len(names) == launches and sum("stage_kernel_het_noise" in n for n in names) == het_launches, (count, names)
        assert not any("stage_kernel_table" in n for n in names), (count, names)
        assert t.host[:16].view(torch.int32).tolist()[2:] == [count, 0]
