"""The host half of mask-blend rows in the table-driven launch (DPM_TABLE_BLEND, C ABI version 211): the real library's
DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_host.py / test_table_sde_host.py.  With the flag every
DPM_F_BLEND request that passes blend_row_ok owns a row from ONE member on and, in a section of its own behind the rows (and
behind the noise records of a DPM_TABLE_NOISE call), a 48-byte blend record: mask, blend_a, blend_b, the 64-bit period, the
bits of blend_alpha / blend_sigma, two zero words.  Without the flag the call is version 210's.

Nothing here launches a kernel.  DPM_TABLE_LAUNCH is only called where it ends before its first launch -- an argument error, or
empty requests: the requests carry CPU addresses.  FILL and LAUNCH group in ONE function of the library; that a launch reads
row i of the run FILL wrote for it is what tests/test_gpu_table_blend.py shows row by row on the device."""
import ctypes as C

import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_host import FIELDS, HDR, POISON, ROW

N = 6144                                   # elements of a request: whole tiles, a multiple of 12 and of 8
NZ, BL = int(L.lib.dpm_sizeof(10)), int(L.lib.dpm_sizeof(12))
FILL_B, LAUNCH_B = L.TABLE_FILL | L.TABLE_BLEND, L.TABLE_LAUNCH | L.TABLE_BLEND
FORMS = (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3)


class Call:
    """kinds[r]: "plain" (an ODE request), "blend" (a qualifying DPM_F_BLEND request: forms LIN1 / TWO / MS3, periods N, N/4
    and 8, blend_b null for every fifth, scalars of its own), "denoise" / "p12" / "misaligned" / "sde" (DPM_F_BLEND requests
    that do not qualify: a DENOISE stage, a period of 12, a mask 8 bytes off, DPM_F_NOISE next to the blend); a kind may carry
    a suffix that keeps its group apart: ":f32" (dtype) or ":cfg" (guidance).  CPU addresses only, never dereferenced."""

    def __init__(self, kinds, noise_section=False):
        R = self.R = len(kinds)
        self.kinds = kinds
        self.st, self.bs = (L.Stage * R)(), (L.Buffers * R)()
        self.arena = np.zeros(64, dtype=np.uint8)
        p0 = (self.arena.ctypes.data + 63) // 64 * 64              # addresses only: spaced 2^20 bytes apart, 64-byte aligned
        for r, kind in enumerate(kinds):
            kind, _, tag = kind.partition(":")
            s, b = self.st[r], self.bs[r]
            s.index, s.form = r % 7, FORMS[(r // 2) % 3]
            s.flags = L.F_TO_X0 | (L.F_STORE_M if r % 2 else 0)
            s.model_type, s.guidance = L.MODEL["noise"], L.GUIDE["uncond"]
            s.alpha_e, s.sigma_e = 0.75 + 0.001 * r, 0.5 - 0.001 * r
            s.cx, s.c0, s.c1, s.c2 = 0.9, -0.1 - 0.01 * r, 0.05, 0.01
            s.k[0] = 0.5
            p = [p0 + ((r * 16 + k) << 20) for k in range(12)]
            b.x, b.e0, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[3], p[4], p[5], p[6]
            b.n, b.batch = N, 1
            b.state_dtype = b.eps_dtype = L.DTYPE_F32 if tag == "f32" else L.DTYPE_F16
            if tag == "cfg":
                s.guidance, s.cfg_scale = L.GUIDE["classifier-free"], 3.0
                b.e1, b.x_out2 = p[2], (p[7] if r % 2 else None)
            if kind != "plain":
                s.flags |= L.F_BLEND
                s.blend_alpha, s.blend_sigma = 0.25 + 0.0078125 * r, 0.5 - 0.00390625 * r
                b.mask, b.blend_a, b.blend_b = p[8], p[9], (None if r % 5 == 4 else p[10])
                b.mask_period = (N, N // 4, 8)[(r // 3) % 3]
            if kind == "denoise":
                s.form = L.FORM_DENOISE
            elif kind == "p12":
                b.mask_period = 12
            elif kind == "misaligned":
                b.mask += 8
            elif kind == "sde":
                s.form, s.flags = FORMS[r % 2], s.flags | L.F_NOISE
        self.opts = L.LaunchOpts()
        self.opts.per_request_stages = 1
        self.bs[0].opts = C.pointer(self.opts)
        self.rec0 = HDR + R * ROW + (R * NZ if noise_section else 0)
        self.size = self.rec0 + R * BL
        self.table = np.full(self.size + 64 + 16, POISON, dtype=np.uint8)      # 64 guard bytes behind the last record
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def run(self, mode):
        self.opts.table_mode = mode
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, None)
        return rc, L.lib.dpm_last_error().decode()

    def fill(self, mode=FILL_B):
        rc, msg = self.run(mode)
        assert rc == 0, (rc, msg)
        return self

    def bytes(self):
        return self.table[self.toff:]

    def header(self):
        return [int(v) for v in self.bytes()[:16].view(np.uint32)]

    def members(self, kind):
        return [r for r, k in enumerate(self.kinds) if k == kind]

    def poison(self, lo, hi):
        return bool((self.bytes()[lo:hi] == POISON).all())

    def check_run(self, first, members, blend=True):
        """rows [first, first + len(members)) are those of `members`, in order; with `blend` so are their records, field by
        field, else the records beside them are untouched"""
        cnt = len(members)
        body = self.bytes()[HDR + first * ROW:HDR + (first + cnt) * ROW].reshape(cnt, ROW)
        ptr, words = body[:, :64].copy().view(np.uint64), body[:, 64:].copy().view(np.uint32)
        assert np.array_equal(ptr, np.array([[getattr(self.bs[r], f) or 0 for f in FIELDS] for r in members], dtype=np.uint64))
        assert np.array_equal(words[:, 0].view(np.float32), np.array([self.st[r].alpha_e for r in members], dtype=np.float32))
        assert words[:, 1].tolist() == [self.st[r].flags for r in members]
        assert words[:, 5].tolist() == [self.st[r].form for r in members]
        lo, hi = self.rec0 + first * BL, self.rec0 + (first + cnt) * BL
        if not blend:
            assert self.poison(lo, hi), "the blend records of rows without a blend were written"
            return
        rec = self.bytes()[lo:hi].reshape(cnt, BL)
        p64 = rec[:, :32].copy().view(np.uint64)
        assert p64[:, 0].tolist() == [self.bs[r].mask for r in members]
        assert p64[:, 1].tolist() == [self.bs[r].blend_a for r in members]
        assert p64[:, 2].tolist() == [self.bs[r].blend_b or 0 for r in members]
        assert p64[:, 3].tolist() == [self.bs[r].mask_period for r in members]
        f32 = rec[:, 32:40].copy().view(np.float32)
        assert np.array_equal(f32[:, 0], np.array([self.st[r].blend_alpha for r in members], dtype=np.float32))
        assert np.array_equal(f32[:, 1], np.array([self.st[r].blend_sigma for r in members], dtype=np.float32))
        assert not rec[:, 40:].any(), "the two trailing words of a blend record are zero"


def test_abi_211_sizes_and_binding():
    assert L.lib.dpm_version() >= 211
    assert BL == 48 == L.TABLE_BLEND_BYTES and L.TABLE_BLEND == 32 and L.lib.dpm_sizeof(11) == 0
    assert (HDR, ROW, NZ) == (16, 144, 32)                                      # as in version 210
    assert C.sizeof(L.Buffers) == L.lib.dpm_sizeof(1) == 184 and C.sizeof(L.LaunchOpts) == L.lib.dpm_sizeof(5) == 32
    valid = [m | f for f in (0, 4, 8, 12, 32, 36, 40, 44) for m in (1, 2)]
    for mode in list(range(-1, 50)) + [64, 65, 66]:
        if mode == 0 or mode in valid:                                          # (no valid LAUNCH of CPU addresses)
            continue
        c = Call(["blend"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)
    for mode in valid:
        if mode & 1:
            assert Call(["plain"] * 20).fill(mode).header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 20, 1], mode


# blend groups of 40, 17, 2 and 1 members among plain rows: kept apart by dtype, guidance kind and model type, opened in call order
def test_blend_groups_of_40_17_2_and_1_among_plain_rows():
    kinds = (["blend", "blend", "plain"] * 20 + ["blend:f32"] * 17 + ["plain"] * 3 + ["blend:cfg"] * 2 + ["plain:f32"] * 5
             + ["blend:f32"])
    c = Call(kinds)
    last = len(kinds) - 1
    c.st[last].model_type = L.MODEL["v"]                       # agrees with no other request: a group of one
    c.fill()
    b40, plain = c.members("blend"), c.members("plain")
    b17 = c.members("blend:f32")[:-1]
    b2 = c.members("blend:cfg")
    assert (len(b40), len(plain), len(b17), len(b2)) == (40, 23, 17, 2)
    # runs in the order their groups open: blend x 40 (request 0), plain x 23 (request 1), f32 blend x 17, cfg blend x 2,
    # the lone v-prediction blend; the five plain f32 requests are a group of 5 without rows
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(kinds), 5]
    c.check_run(0, b40)
    c.check_run(40, plain, blend=False)
    c.check_run(63, b17)
    c.check_run(80, b2)
    c.check_run(82, [last])
    assert c.poison(HDR + 83 * ROW, c.rec0), "rows behind the last run were written"
    assert c.poison(c.rec0 + 83 * BL, c.size + 64), "records behind the last run were written"
    # the rotation is there: three forms, null and non-null blend_b, three periods in ONE group
    assert {c.st[r].form for r in b40} == set(FORMS)
    assert {bool(c.bs[r].blend_b) for r in b40} == {True, False}
    assert {c.bs[r].mask_period for r in b40} == {N, N // 4, 8}


@pytest.mark.parametrize("bad", ["denoise", "p12", "misaligned", "sde"])
def test_a_blend_request_that_does_not_qualify_owns_no_row(bad):
    kinds = ["blend"] * 10 + [bad] + ["blend"] * 9
    c = Call(kinds).fill()
    assert c.header()[2:] == [20, 1]
    c.check_run(0, c.members("blend"))
    assert c.poison(HDR + 19 * ROW, c.rec0) and c.poison(c.rec0 + 19 * BL, c.size + 64)
    # ... alone in a call it writes no row at all
    c = Call([bad]).fill()
    assert c.header()[2:] == [1, 0] and c.poison(HDR, c.size + 64)


def test_the_blend_section_sits_behind_the_noise_section():
    kinds = ["blend"] * 3 + ["plain"] * 2
    c = Call(kinds, noise_section=True)
    for r in (3, 4):                                           # two SDE requests: rows and noise records with DPM_TABLE_NOISE
        c.st[r].form, c.st[r].flags = L.FORM_LIN1, c.st[r].flags | L.F_NOISE
    c.fill(FILL_B | L.TABLE_NOISE)
    assert c.header()[2:] == [5, 2] and c.rec0 == HDR + 5 * ROW + 5 * NZ
    c.check_run(0, [0, 1, 2])
    c.check_run(3, [3, 4], blend=False)
    nz0 = HDR + 5 * ROW
    assert c.poison(nz0, nz0 + 3 * NZ), "the noise records of the blend rows were written"
    rec = c.bytes()[nz0 + 3 * NZ:nz0 + 5 * NZ].copy().view(np.uint32).reshape(2, 8)
    assert rec[:, 2].tolist() == [c.st[3].index, c.st[4].index] and not rec[:, 4:].any()
    assert c.poison(c.size, c.size + 64)


def test_the_flag_on_a_call_without_a_blend_stage_changes_nothing():
    kinds = ["plain"] * 20 + ["plain:f32"] * 18 + ["plain:cfg"] * 3
    a, b = Call(kinds).fill(L.TABLE_FILL), Call(kinds).fill(FILL_B)
    assert a.header()[2:] == [41, 2]
    # (the two calls differ in their addresses by the distance of their arenas: compare rows relative to request 0's x)
    ra, rb = a.bytes()[HDR:HDR + 38 * ROW].reshape(38, ROW), b.bytes()[HDR:HDR + 38 * ROW].reshape(38, ROW)
    pa, pb = ra[:, :64].copy().view(np.uint64), rb[:, :64].copy().view(np.uint64)
    assert np.array_equal(np.where(pa != 0, pa - np.uint64(a.bs[0].x), 0), np.where(pb != 0, pb - np.uint64(b.bs[0].x), 0))
    assert np.array_equal(ra[:, 64:], rb[:, 64:]) and np.array_equal(a.bytes()[:16], b.bytes()[:16])
    assert a.poison(HDR + 38 * ROW, a.size + 64) and b.poison(HDR + 38 * ROW, b.size + 64)


def test_without_the_flag_the_call_is_version_210s():
    kinds = ["blend", "plain"] * 20
    c = Call(kinds).fill(L.TABLE_FILL)
    # blend requests take their mode-0 path -- no rows, no records --, the 20 plain requests are the one run
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 40, 1]
    c.check_run(0, c.members("plain"), blend=False)
    assert c.poison(HDR + 20 * ROW, c.size + 64)
    c = Call(["blend"] * 20).fill(L.TABLE_FILL | L.TABLE_NOISE | L.TABLE_THRESH)
    assert c.header()[2:] == [20, 0] and c.poison(HDR, c.size + 64)


def test_fill_and_launch_check_alike_and_end_before_a_launch_alike():
    for mode in (FILL_B, LAUNCH_B):
        # check_stage_buffers keeps its blend argument rules, with the texts of mode 0, and nothing is written
        for edit, text in ((lambda c: setattr(c.bs[7], "mask", None), "DPM_F_BLEND needs mask"),
                           (lambda c: setattr(c.bs[7], "mask_period", 7), "not a multiple of mask_period"),
                           (lambda c: setattr(c.bs[7], "blend_a", None), "DPM_F_BLEND needs mask")):
            c = Call(["blend"] * 20)
            edit(c)
            before = c.table.copy()
            rc, msg = c.run(mode)
            assert rc == L.ERR_ARG and text in msg, (mode, rc, msg)
            assert np.array_equal(c.table, before), "a refused call wrote into the table"
        # empty requests own no rows and launch nothing in either mode
        c = Call(["blend"] * 20)
        for r in range(20):
            c.bs[r].n = 0
        before = c.table.copy()
        assert c.run(mode)[0] == 0
        if mode == FILL_B:
            assert c.header()[2:] == [20, 0] and c.poison(HDR, c.size + 64)
        else:
            assert np.array_equal(c.table, before)
