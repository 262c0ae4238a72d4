"""The host half of SDE rows in the table-driven launch (DPM_TABLE_NOISE, dpm_buffers.noise_sample0, C ABI version 209): the
real library's DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_host.py.  With the flag every fusable
SDE request owns a row and, behind the n_req rows the table has room for, a 32-byte noise record -- seed, stage index, scale
and the 64-bit base of the row's Philox block indices; without it the call is version 208's.  Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_host import FIELDS, HDR, N, POISON, ROW

NZ = int(L.lib.dpm_sizeof(10))
FILL_N, LAUNCH_N = L.TABLE_FILL | L.TABLE_NOISE, L.TABLE_LAUNCH | L.TABLE_NOISE


class Call:
    """n_req well-formed requests with CPU pointers (never dereferenced); kinds[r] = "sde" or "ode"; SDE requests rotate
    LIN1 / TWO and carry their own seed (an options struct each), index, c2 and noise_sample0 = r % 4"""

    def __init__(self, kinds, n=N, base=lambda r: r % 4):
        R = self.R = len(kinds)
        self.st, self.bs = (L.Stage * R)(), (L.Buffers * R)()
        self.arena = np.zeros(64, dtype=np.uint8)
        p0 = (self.arena.ctypes.data + 63) // 64 * 64              # addresses only: spaced 2^20 bytes apart, 16-byte aligned
        self.ropts = [L.LaunchOpts() for _ in range(R)]
        for r, kind in enumerate(kinds):
            s, b = self.st[r], self.bs[r]
            s.index, s.form = 3 + r, (L.FORM_LIN1, L.FORM_TWO)[r % 2]
            s.flags = L.F_TO_X0 | L.F_STORE_M | (L.F_NOISE if kind == "sde" else 0)
            s.model_type, s.guidance = L.MODEL["noise"], L.GUIDE["uncond"]
            s.alpha_e, s.sigma_e = 0.75 + 0.001 * r, 0.5 - 0.001 * r
            s.cx, s.c0, s.c1, s.c2 = 0.9, -0.1 - 0.01 * r, 0.05, 0.25 + 0.015625 * r
            s.k[0] = 0.5
            p = [p0 + ((r * 8 + k) << 20) for k in range(8)]
            b.x, b.e0, b.h1, b.x_out, b.m_out = p[0], p[1], p[3], p[5], p[6]
            b.n, b.batch = n, 1
            b.state_dtype = b.eps_dtype = L.DTYPE_F16
            if kind == "sde":
                self.ropts[r].noise_seed_lo, self.ropts[r].noise_seed_hi = 0x1000 + r, 0xABCD0000 + 7 * r
                b.opts = C.pointer(self.ropts[r])
                b.noise_sample0 = base(r)
        self.opts = L.LaunchOpts()
        C.memmove(C.byref(self.opts), C.byref(self.ropts[0]), C.sizeof(L.LaunchOpts))      # request 0's seed, the call's flags
        self.opts.per_request_stages = 1
        self.bs[0].opts = C.pointer(self.opts)
        self.size = HDR + R * (ROW + NZ)
        self.table = np.full(self.size + 64 + 16, POISON, dtype=np.uint8)      # 64 guard bytes behind the last record
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def run(self, mode):
        self.opts.table_mode = mode
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, None)
        return rc, L.lib.dpm_last_error().decode()

    def fill(self, mode=FILL_N):
        rc, msg = self.run(mode)
        assert rc == 0, (rc, msg)
        return self

    def bytes(self):
        return self.table[self.toff:]

    def header(self):
        return [int(v) for v in self.bytes()[:16].view(np.uint32)]

    def rows(self, first, count):
        body = self.bytes()[HDR + first * ROW:HDR + (first + count) * ROW].reshape(count, ROW)
        return body[:, :64].copy().view(np.uint64), body[:, 64:].copy().view(np.uint32)

    def records(self, first, count):
        o = HDR + self.R * ROW + first * NZ
        return self.bytes()[o:o + count * NZ].copy().view(np.uint32).reshape(count, 8)

    def pointers(self, members):
        return np.array([[getattr(self.bs[r], f) or 0 for f in FIELDS] for r in members], dtype=np.uint64)

    def want_records(self, members):
        out = []
        for r in members:
            g0 = self.bs[r].noise_sample0 * (self.bs[r].n // self.bs[r].batch) // 4
            out.append([self.ropts[r].noise_seed_lo, self.ropts[r].noise_seed_hi, self.st[r].index,
                        int(np.float32(self.st[r].c2).view(np.uint32)), g0 & 0xffffffff, g0 >> 32, 0, 0])
        return np.array(out, dtype=np.uint32)

    def poison(self, lo, hi):
        return bool((self.bytes()[lo:hi] == POISON).all())

    def check_run(self, first, members):
        """rows [first, first + len(members)) and their records are those of `members`, in order"""
        ptr, words = self.rows(first, len(members))
        assert np.array_equal(ptr, self.pointers(members))
        assert np.array_equal(words[:, 0].view(np.float32), np.array([self.st[r].alpha_e for r in members], dtype=np.float32))
        assert words[:, 1].tolist() == [self.st[r].flags for r in members]
        assert words[:, 5].tolist() == [self.st[r].form for r in members]


def test_abi_209_sizes_and_binding():
    assert L.lib.dpm_version() >= 209
    assert C.sizeof(L.Buffers) == L.lib.dpm_sizeof(1) == 184 and C.sizeof(L.LaunchOpts) == L.lib.dpm_sizeof(5) == 32
    assert L.Buffers.noise_sample0.offset == L.Buffers.reserved.offset == L.Buffers.inputs_resident.offset + 4
    assert L.Buffers.thr_hint.offset == L.Buffers.noise_sample0.offset + 4
    b = L.Buffers()
    b.reserved = 7
    assert b.noise_sample0 == 7
    assert NZ == 32 == L.TABLE_NOISE_BYTES and L.TABLE_NOISE == 4 and L.lib.dpm_sizeof(9) == 0
    for mode in (4, 3, 7, -1):
        c = Call(["sde"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg, (rc, msg)
        assert np.array_equal(c.table, before)


def test_fill_writes_rows_and_noise_records():
    c = Call(["sde"] * 20).fill()
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 20, 1]
    c.check_run(0, range(20))
    assert np.array_equal(c.records(0, 20), c.want_records(range(20)))
    assert c.records(0, 20)[:, 4].tolist() == [(r % 4) * N // 4 for r in range(20)]
    assert c.poison(c.size, c.size + 64), "bytes behind the last record were written"


def test_the_high_word_of_the_base():
    c = Call(["sde"] * 20, n=1 << 14, base=lambda r: (1 << 21) + r if r % 2 else 0).fill()
    rec = c.records(0, 20)
    assert np.array_equal(rec, c.want_records(range(20)))
    g0 = ((1 << 21) + 1) * (1 << 14) // 4
    assert g0 >= 1 << 32 and rec[1, 4:6].tolist() == [g0 & 0xffffffff, g0 >> 32] and rec[1, 5] == 2 and rec[0, 4:6].tolist() == [0, 0]


@pytest.mark.parametrize("R", [2, 1])
def test_small_sde_groups_get_rows(R):
    c = Call(["sde"] * R).fill()
    assert c.header()[2:] == [R, 1]
    c.check_run(0, range(R))
    assert np.array_equal(c.records(0, R), c.want_records(range(R)))
    assert c.poison(c.size, c.size + 64)


def test_ode_and_sde_groups_are_two_runs():
    kinds = [("ode", "sde")[r % 2] for r in range(40)]
    c = Call(kinds).fill()
    assert c.header()[2:] == [40, 2]
    ode, sde = list(range(0, 40, 2)), list(range(1, 40, 2))
    c.check_run(0, ode)
    c.check_run(20, sde)
    rec0 = HDR + 40 * ROW
    assert c.poison(rec0, rec0 + 20 * NZ), "the records of the ODE rows were written"
    assert np.array_equal(c.records(20, 20), c.want_records(sde))
    assert c.poison(HDR + 40 * ROW + 40 * NZ, c.size + 64) and c.poison(rec0 + 40 * NZ, c.size + 64)


def test_a_small_ode_group_writes_no_rows_beside_three_sde_rows():
    c = Call(["ode"] * 10 + ["sde"] * 3).fill()
    assert c.header()[2:] == [13, 1]
    c.check_run(0, [10, 11, 12])
    assert np.array_equal(c.records(0, 3), c.want_records([10, 11, 12]))
    assert c.poison(HDR + 3 * ROW, HDR + 13 * ROW) and c.poison(HDR + 13 * ROW + 3 * NZ, c.size + 64)


def test_without_the_flag_the_call_is_version_208s():
    c = Call(["sde"] * 20, base=lambda r: 0).fill(L.TABLE_FILL)
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 20, 0]
    assert c.poison(HDR, c.size + 64)


def _refused(c, mode, text="noise_sample0"):
    before = c.table.copy()
    rc, msg = c.run(mode)
    assert rc == L.ERR_ARG and text in msg, (mode, rc, msg)
    assert np.array_equal(c.table, before), "a refused call wrote into the table"


def test_every_argument_error_of_noise_sample0():
    for mode in (0, L.TABLE_FILL, L.TABLE_LAUNCH):                 # honoured by table noise rows only
        _refused(Call(["sde"] * 20), mode)
    c = Call(["sde"] * 20, base=lambda r: 0)                       # a lone launch, too (refused before anything is launched)
    c.bs[3].noise_sample0 = 1
    assert L.lib.dpm_stage_launch(C.byref(c.st[3]), C.byref(c.bs[3]), None) == L.ERR_ARG
    assert "noise_sample0" in L.lib.dpm_last_error().decode()
    for mode in (FILL_N, LAUNCH_N):
        c = Call(["sde"] * 10 + ["ode"] * 10, base=lambda r: 0)
        c.bs[15].noise_sample0 = 2
        _refused(c, mode, "without DPM_F_NOISE")
        c = Call(["sde"] * 20)
        c.bs[6].x_out += 8                                         # unaligned: fits no fused group
        _refused(c, mode, "fits no fused group")
        _refused(Call(["sde"] * 20, n=2044), mode, "fits no fused group")      # n % 8 != 0
        c = Call(["sde"] * 20)
        c.bs[5].noise_sample0 = -1
        _refused(c, mode, "negative")
        c = Call(["sde"] * 20, n=2056)                             # 2056 elements: bases are whole blocks ...
        c.fill()
        c = Call(["sde"] * 20, n=2056)
        c.bs[9].batch, c.bs[9].noise_sample0 = 4, 1                # ... 514 per sample: sample 1 starts inside a block
        _refused(c, mode, "multiple of 4")
