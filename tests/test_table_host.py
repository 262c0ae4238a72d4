"""The host half of the table-driven heterogeneous launch (dpm_launch_opts.table_mode, C ABI version 208): the real library
through ctypes, no GPU.  DPM_TABLE_FILL checks and groups the requests of a per-request-stage call and writes the table -- a
header and, for every group of more than 16 members, a run of rows in call order -- without launching anything or calling
into HIP, so this file walks it with CPU pointers.  Nothing here launches a kernel: the mode-0 calls it makes are calls
that end before any launch (an argument error, or empty requests)."""
import ctypes as C

import numpy as np
import pytest

from dpm_solver_amd import _lib as L

HDR, ROW = int(L.lib.dpm_sizeof(7)), int(L.lib.dpm_sizeof(8))
N = 2048                                   # elements of a request
POISON = 0xAB
FIELDS = ("x", "e0", "e1", "h1", "h2", "x_out", "m_out", "x_out2")        # the pointers of a row, in its order


class Call:
    """n_req well-formed requests with CPU pointers of distinct, 16-byte aligned addresses; forms[r], dtypes[r] per request"""

    def __init__(self, forms, sdt=None, thresh=(), table_bytes=None):
        R = self.R = len(forms)
        self.st, self.bs = (L.Stage * R)(), (L.Buffers * R)()
        self.arena = np.zeros(R * 9 * N * 4 + 64, dtype=np.uint8)      # never read or written by the library
        base = (self.arena.ctypes.data + 63) // 64 * 64
        for r, form in enumerate(forms):
            s, b = self.st[r], self.bs[r]
            s.index, s.form = r % 5, getattr(L, "FORM_" + form)
            s.flags = L.F_TO_X0 | L.F_STORE_M
            if form == "UNIPC":
                s.flags |= L.F_UNIPC_DP if r % 2 else L.F_UNIPC_P2
            s.model_type, s.guidance = L.MODEL["noise"], L.GUIDE["uncond"]
            s.alpha_e, s.sigma_e = 0.75 + 0.001 * r, 0.5 - 0.001 * r
            s.cx, s.c0, s.c1, s.c2 = 0.9, -0.1 - 0.01 * r, 0.05, 0.01
            s.h1_slot, s.h2_slot, s.m_slot = 0, 1, 2
            p = [base + (r * 9 + k) * N * 4 for k in range(9)]
            b.x, b.e0, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[3], p[4], p[5], p[6]
            b.n, b.batch = N, 1
            b.state_dtype = b.eps_dtype = (sdt[r] if sdt else L.DTYPE_F16)
            if r in thresh:
                s.flags |= L.F_THRESH
                s.thr_ratio, s.thr_max = 0.995, 1.0
                b.workspace = p[8]
        self.opts = L.LaunchOpts()
        self.opts.per_request_stages = 1
        self.bs[0].opts = C.pointer(self.opts)
        self.table = np.full((table_bytes or HDR + R * ROW) + 16, POISON, dtype=np.uint8)
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def run(self, mode):
        self.opts.table_mode = mode
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, None)
        return rc, L.lib.dpm_last_error().decode()

    def fill(self):
        rc, msg = self.run(L.TABLE_FILL)
        assert rc == 0, (rc, msg)
        return self

    def bytes(self):
        return self.table[self.toff:self.toff + HDR + self.R * ROW]

    def header(self):
        return [int(v) for v in self.bytes()[:16].view(np.uint32)]

    def rows(self, count):
        """the pointers of the first `count` rows, [count, 8], and their scalar words, [count, (ROW - 64) / 4]"""
        body = self.bytes()[HDR:HDR + count * ROW].reshape(count, ROW)
        return body[:, :64].copy().view(np.uint64), body[:, 64:].copy().view(np.uint32)

    def pointers(self, members):
        return np.array([[getattr(self.bs[r], f) or 0 for f in FIELDS] for r in members], dtype=np.uint64)

    def untouched_from(self, count):
        return bool((self.bytes()[HDR + count * ROW:] == POISON).all())


def test_abi_208_sizes_and_binding():
    assert L.lib.dpm_version() >= 208
    assert C.sizeof(L.LaunchOpts) == 32 and L.lib.dpm_sizeof(5) == 32
    assert L.LaunchOpts.table_mode.offset == 28 and L.LaunchOpts().table_mode == 0
    assert HDR > 0 and ROW > 0 and HDR % 16 == 0 and ROW % 16 == 0
    assert (L.TABLE_HEADER_BYTES, L.TABLE_ROW_BYTES) == (HDR, ROW) and (L.TABLE_FILL, L.TABLE_LAUNCH) == (1, 2)
    assert L.lib.dpm_sizeof(9) == 0


@pytest.mark.parametrize("R", [17, 40, 200])
def test_fill_writes_one_run_in_call_order(R):
    c = Call([("LIN1", "TWO")[r % 2] for r in range(R)]).fill()
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
    ptr, words = c.rows(R)
    want = c.pointers(range(R))
    assert np.array_equal(ptr, want)
    for k in (0, 1, 5):                                           # x, e0, x_out: distinct per request
        assert len(set(ptr[:, k].tolist())) == R and not (ptr[:, k] % 16).any()
    # the scalars of a row are the record of ITS request: alpha_e is the first word, the flags the second, the form the sixth
    assert np.array_equal(words[:, 0].view(np.float32), np.array([c.st[r].alpha_e for r in range(R)], dtype=np.float32))
    assert words[:, 1].tolist() == [c.st[r].flags for r in range(R)]
    assert words[:, 5].tolist() == [c.st[r].form for r in range(R)]
    assert c.untouched_from(R)


def test_a_group_of_16_writes_no_rows():
    c = Call(["TWO"] * 16).fill()
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 16, 0]
    assert c.untouched_from(0)
    # ... nor do two groups of 16 and 12: dtypes keep them apart
    c = Call(["TWO"] * 28, sdt=[L.DTYPE_F16] * 16 + [L.DTYPE_F32] * 12).fill()
    assert c.header()[2:] == [28, 0] and c.untouched_from(0)


@pytest.mark.parametrize("odd", ["thresholded", "dtype"])
def test_a_request_outside_the_group_leaves_the_rows_of_the_others(odd):
    forms = [("LIN1", "TWO")[r % 2] for r in range(41)]
    c = Call(forms, thresh={20} if odd == "thresholded" else (),
             sdt=[L.DTYPE_F32 if (r == 20 and odd == "dtype") else L.DTYPE_F16 for r in range(41)]).fill()
    assert c.header()[2:] == [41, 1]
    members = [r for r in range(41) if r != 20]
    ptr, words = c.rows(40)
    assert np.array_equal(ptr, c.pointers(members))
    assert words[:, 0].view(np.float32).tolist() == [c.st[r].alpha_e for r in members]
    assert c.untouched_from(40)


def test_ms3_and_unipc_records_land_in_different_runs():
    forms = [("TWO", "MS3", "UNIPC")[r % 3] for r in range(60)]
    c = Call(forms).fill()
    assert c.header()[2:] == [60, 2]
    first = [r for r in range(60) if r % 3 != 2]                   # the first MS3 record closes the group to UNIPC
    second = [r for r in range(60) if r % 3 == 2]
    ptr, words = c.rows(60)
    assert np.array_equal(ptr, c.pointers(first + second))
    assert set(words[:40, 5].tolist()) == {L.FORM_TWO, L.FORM_MS3} and set(words[40:, 5].tolist()) == {L.FORM_UNIPC}
    # 34 TWO records, then 20 UNIPC, then 3 MS3: TWO joins the UniPC run, the MS3 records are a group of 3 without rows
    forms = ["TWO"] * 34 + ["UNIPC"] * 20 + ["MS3"] * 3
    c = Call(forms).fill()
    assert c.header()[2:] == [57, 1]
    assert np.array_equal(c.rows(54)[0], c.pointers(range(54))) and c.untouched_from(54)


def _refused(c, mode, text):
    before = c.table.copy()
    rc, msg = c.run(mode)
    assert rc == L.ERR_ARG and text in msg, (rc, msg)
    assert np.array_equal(c.table, before), "a refused call wrote into the table"


def test_every_argument_error_of_table_mode():
    forms = ["TWO"] * 20
    for mode in (3, -1, 7):
        _refused(Call(forms), mode, "table_mode=%d" % mode)
    for mode in (L.TABLE_FILL, L.TABLE_LAUNCH):
        c = Call(forms)
        c.opts.per_request_stages = 0
        _refused(c, mode, "per_request_stages")
        c = Call(forms)
        c.opts.fuse_shapes = 1
        _refused(c, mode, "fuse_shapes")
        c = Call(forms)
        c.bs[0].workspace = None
        _refused(c, mode, "bs[0].workspace")
        c = Call(forms)
        c.bs[0].workspace += 8
        _refused(c, mode, "16-byte aligned")
        _refused(Call(forms, thresh={0}), mode, "DPM_F_THRESH in st[0]")
        # a request's own error: the text of mode 0, nothing written, nothing launched
        c = Call(forms)
        c.bs[11].e0 = None
        _refused(c, mode, "e0 / x_out must not be null")
        c = Call(forms)
        c.st[7].form, c.bs[7].h2 = L.FORM_MS3, None
        _refused(c, mode, "needs h2")


def test_mode_0_on_the_same_arrays_is_the_call_it_was():
    c = Call(["TWO"] * 20)
    c.bs[11].e0 = None
    _refused(c, 0, "e0 / x_out must not be null")                 # the same check, the same text, without a table
    c = Call(["TWO"] * 20)
    for r in range(20):
        c.bs[r].n = 0                                             # empty requests: DPM_OK before any launch, as before 208
    before = c.table.copy()
    assert c.run(0)[0] == 0 and np.array_equal(c.table, before)
    assert c.run(L.TABLE_FILL)[0] == 0 and c.header()[2:] == [20, 0] and c.untouched_from(0)
    # the word was `reserved[0]` until 207: the binding keeps that name on the same bytes
    assert L.LaunchOpts.reserved.offset == L.LaunchOpts.table_mode.offset == 28
