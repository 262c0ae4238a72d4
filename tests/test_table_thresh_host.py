"""The host half of thresholded rows in the table-driven launch (DPM_TABLE_THRESH, C ABI version 210): the real library's
DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_host.py.  With the flag every thresholded request whose
sample fits one workgroup owns a row, from a group of one on, in runs of its own; without it the call is version 209's.
Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_host import FIELDS, HDR, N, POISON, ROW

THR = L.TABLE_THRESH
VALID = (1, 2, 5, 6, 9, 10, 13, 14)


class Call:
    """n_req well-formed requests with CPU pointers (never dereferenced); kinds[r] = "thr" or "ode"; forms rotate over
    LIN1 / TWO / MS3.  Thresholded requests carry NO workspace; `table_bytes` leaves room for a noise section."""

    def __init__(self, kinds, n=N, batch=1):
        R = self.R = len(kinds)
        self.st, self.bs = (L.Stage * R)(), (L.Buffers * R)()
        self.arena = np.zeros(64, dtype=np.uint8)
        p0 = (self.arena.ctypes.data + 63) // 64 * 64              # addresses only: spaced 2^20 bytes apart, 16-byte aligned
        for r, kind in enumerate(kinds):
            s, b = self.st[r], self.bs[r]
            s.index, s.form = r % 5, (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3)[r % 3]
            s.flags = L.F_TO_X0 | (L.F_STORE_M if r % 2 else 0) | (L.F_THRESH if kind == "thr" else 0)
            s.model_type, s.guidance = L.MODEL["noise"], L.GUIDE["uncond"]
            s.alpha_e, s.sigma_e = 0.75 + 0.001 * r, 0.5 - 0.001 * r
            s.cx, s.c0, s.c1, s.c2 = 0.9, -0.1 - 0.01 * r, 0.05, 0.01
            s.thr_ratio, s.thr_max = 0.995, 1.0
            p = [p0 + ((r * 8 + k) << 20) for k in range(8)]
            b.x, b.e0, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[3], p[4], p[5], p[6]
            b.n, b.batch = n * batch, batch
            b.state_dtype = b.eps_dtype = L.DTYPE_F16
        self.opts = L.LaunchOpts()
        self.opts.per_request_stages = 1
        self.bs[0].opts = C.pointer(self.opts)
        self.size = HDR + R * (ROW + L.TABLE_NOISE_BYTES)
        self.table = np.full(self.size + 64 + 16, POISON, dtype=np.uint8)
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def run(self, mode):
        self.opts.table_mode = mode
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, None)
        return rc, L.lib.dpm_last_error().decode()

    def fill(self, mode=L.TABLE_FILL | THR):
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

    def poison(self, lo, hi=None):
        return bool((self.bytes()[lo:self.size + 64 if hi is None else hi] == POISON).all())

    def check_run(self, first, members):
        """rows [first, first + len(members)) are those of `members`, in order: pointers, alpha_e, flags, form"""
        ptr, words = self.rows(first, len(members))
        want = np.array([[getattr(self.bs[r], f) or 0 for f in FIELDS] for r in members], dtype=np.uint64)
        assert np.array_equal(ptr, want)
        assert np.array_equal(words[:, 0].view(np.float32), np.array([self.st[r].alpha_e for r in members], dtype=np.float32))
        assert words[:, 1].tolist() == [self.st[r].flags for r in members]
        assert words[:, 5].tolist() == [self.st[r].form for r in members]


def test_abi_210_and_the_modes():
    assert L.lib.dpm_version() >= 210
    assert THR == 8 and (L.TABLE_FILL, L.TABLE_LAUNCH, L.TABLE_NOISE) == (1, 2, 4)
    assert (int(L.lib.dpm_sizeof(7)), int(L.lib.dpm_sizeof(8)), int(L.lib.dpm_sizeof(10))) == (16, 144, 32)   # as in version 209
    assert L.lib.dpm_sizeof(9) == 0 and L.lib.dpm_sizeof(11) == 0              # a thresholded row needs no record of its own
    for mode in range(-1, 18):
        if mode in VALID or mode == 0:
            continue
        c = Call(["thr"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)
    for mode in (1, 5, 9, 13):                                                  # every valid FILL mode fills (no HIP call)
        c = Call(["ode"] * 20).fill(mode)
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 20, 1]


@pytest.mark.parametrize("mode", [9, 13])
def test_thresholded_and_plain_requests_are_two_runs(mode):
    kinds = [("ode", "thr")[r % 2] for r in range(40)]
    c = Call(kinds).fill(mode)
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 40, 2]
    ode, thr = list(range(0, 40, 2)), list(range(1, 40, 2))
    c.check_run(0, ode)
    c.check_run(20, thr)
    assert {c.st[r].form for r in thr} == {L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3}        # the three forms share the run
    assert c.poison(HDR + 40 * ROW), "bytes behind the rows were written (no record section for thresholded rows)"
    # the thresholded run first when a thresholded request opens the call
    c = Call(kinds[1:] + kinds[:1]).fill(mode)
    assert c.header()[2:] == [40, 2]
    c.check_run(0, list(range(0, 40, 2)))
    assert c.st[0].flags & L.F_THRESH


@pytest.mark.parametrize("R", [1, 2, 17])
def test_a_group_of_one_owns_a_row(R):
    c = Call(["thr"] * R).fill()
    assert c.header()[2:] == [R, 1]
    c.check_run(0, range(R))
    assert c.poison(HDR + R * ROW)
    # ... beside a plain group too small for rows
    c = Call(["ode"] * 10 + ["thr"]).fill()
    assert c.header()[2:] == [11, 1]
    c.check_run(0, [10])
    assert c.poison(HDR + ROW)


def _outsider(kind):
    c = Call(["thr"] * 21)
    if kind == "12296 elements":
        c.bs[7].n = 12296
    elif kind == "thr_ratio":
        c.st[7].thr_ratio = 0.99
    elif kind == "thr_max":
        c.st[7].thr_max = 1.5
    elif kind == "unaligned":
        c.bs[7].x_out += 8
    elif kind == "blend":
        c.st[7].flags |= L.F_BLEND
        c.bs[7].mask, c.bs[7].blend_a, c.bs[7].mask_period = c.bs[7].x, c.bs[7].x, 8
    return c


@pytest.mark.parametrize("kind", ["12296 elements", "thr_ratio", "thr_max", "unaligned", "blend"])
def test_a_request_outside_the_group_leaves_the_rows_of_the_others(kind):
    c = _outsider(kind).fill()
    others = [r for r in range(21) if r != 7]
    ref = Call(["thr"] * 21).fill()                                # the same 20 rows as without the outsider
    lone_row = kind in ("thr_ratio", "thr_max")                    # a group of one of its own: the second run
    assert c.header()[2:] == [21, 2 if lone_row else 1]
    c.check_run(0, others)
    want_ptr, want_words = ref.rows(0, 21)
    got_ptr, got_words = c.rows(0, 20)
    keep = np.array(others)
    assert np.array_equal(got_words, want_words[keep])
    if lone_row:
        c.check_run(20, [7])
    assert c.poison(HDR + (21 if lone_row else 20) * ROW)


def test_12288_elements_fit_and_batches_of_three():
    c = Call(["thr"] * 3, n=12288).fill()
    assert c.header()[2:] == [3, 1]
    c = Call(["thr"] * 3, n=4096, batch=3).fill()                  # n = 12288 over three samples of 4096
    assert c.header()[2:] == [3, 1]
    c = Call(["thr"] * 3, n=12288, batch=3).fill()                 # n / batch is what has to fit
    assert c.header()[2:] == [3, 1]
    c = Call(["thr"] * 3, n=12296)                                # request 0 is no row: its lone launch needs a workspace, not the table
    rc, msg = c.run(L.TABLE_FILL | THR)
    assert rc == L.ERR_ARG and "DPM_F_THRESH in st[0]" in msg, (rc, msg)


@pytest.mark.parametrize("per,batch", [(10, 4), (2, 4), (6, 4), (2058, 4)])
def test_a_request_whose_sample_is_no_multiple_of_4_gets_no_row(per, batch):
    """n = batch x per is a multiple of 8, the sample is not a multiple of 4: the kernel works per sample in 4-element
    accesses, so such a request takes its mode-0 path -- alone, and beside requests that own rows"""
    assert (per * batch) % 8 == 0 and per % 4 != 0
    c = Call(["ode"] + ["thr"] * 3, n=per, batch=batch)
    for r in range(1, 4):
        c.bs[r].workspace = c.bs[r].x                              # (their lone launches' workspaces)
    c.fill()
    assert c.header()[2:] == [4, 0] and c.poison(HDR), "a request of ragged samples wrote a row"
    rc, msg = Call(["thr"] * 3, n=per, batch=batch).run(L.TABLE_FILL | THR)           # as st[0]: refused, as without the flag
    assert rc == L.ERR_ARG and "DPM_F_THRESH in st[0]" in msg, (rc, msg)
    c = Call(["thr"] * 6, n=per * batch)                           # five requests of ONE sample of the same n: rows ...
    c.bs[3].batch = batch                                          # ... the one of `batch` ragged samples: none
    c.fill()
    assert c.header()[2:] == [6, 1]
    c.check_run(0, [0, 1, 2, 4, 5])
    assert c.poison(HDR + 5 * ROW)
    # whole 4-element samples of a batch do own rows, down to 4 elements
    for ok_per, ok_batch in ((4, 2), (12, 2), (8, 3), (2052, 2)):
        c = Call(["thr"] * 2, n=ok_per, batch=ok_batch).fill()
        assert c.header()[2:] == [2, 1], (ok_per, ok_batch)


def test_the_thresholded_denoise_stage_owns_a_row_in_the_group_of_the_other_forms():
    """DPM_FORM_DENOISE + DPM_F_THRESH (the last stage of denoise_to_zero): a row like the others, no h1 / h2, in call order"""
    c = Call(["thr"] * 9)
    for r in (0, 4, 8):
        c.st[r].form = L.FORM_DENOISE
        c.bs[r].h1 = c.bs[r].h2 = None
    c.fill()
    assert c.header()[2:] == [9, 1]
    c.check_run(0, range(9))
    assert c.rows(0, 9)[1][:, 5].tolist().count(L.FORM_DENOISE) == 3 and c.poison(HDR + 9 * ROW)
    c = Call(["thr"])                                              # ... and alone
    c.st[0].form = L.FORM_DENOISE
    c.fill()
    assert c.header()[2:] == [1, 1]
    # without DPM_F_THRESH a DENOISE stage stays outside every fused group, with and without the flag
    c = Call(["ode"] * 20)
    c.st[5].form = L.FORM_DENOISE
    c.fill()
    assert c.header()[2:] == [20, 1]
    c.check_run(0, [r for r in range(20) if r != 5])


def test_without_the_flag_every_call_is_version_209s():
    kinds = [("ode", "thr")[r % 2] for r in range(40)]
    kinds[0], kinds[1] = "ode", "ode"
    for mode in (L.TABLE_FILL, L.TABLE_FILL | L.TABLE_NOISE):
        c = Call(kinds)
        for r in range(40):
            if kinds[r] == "thr":
                c.bs[r].workspace = c.bs[r].x                       # (their lone launches' workspaces: not the library's to judge)
        c.fill(mode)
        ode = [r for r in range(40) if kinds[r] == "ode"]
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 40, 1]
        c.check_run(0, ode)
        assert c.poison(HDR + len(ode) * ROW), "a thresholded request wrote a row without DPM_TABLE_THRESH"
        # ... and the rows of the plain requests are byte for byte those the flag leaves them
        was = c.bytes()[HDR:HDR + len(ode) * ROW].copy()
        c.table[:] = POISON
        c.fill(mode | THR)
        assert c.header()[2:] == [40, 2] and np.array_equal(c.bytes()[HDR:HDR + len(ode) * ROW], was)


def test_st0_thresholded_is_accepted_with_the_flag_and_refused_without():
    for mode in (L.TABLE_FILL, L.TABLE_LAUNCH, L.TABLE_FILL | L.TABLE_NOISE):
        c = Call(["thr"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "DPM_F_THRESH in st[0]" in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)
    for mode in (9, 13):
        c = Call(["thr"] * 20).fill(mode)
        assert c.header()[2:] == [20, 1]
    # a request's own error keeps mode 0's text, and nothing is written
    c = Call(["thr"] * 20)
    c.bs[11].e0 = None
    before = c.table.copy()
    rc, msg = c.run(L.TABLE_FILL | THR)
    assert rc == L.ERR_ARG and "e0 / x_out must not be null" in msg and np.array_equal(c.table, before)
