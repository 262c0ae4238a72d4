"""The host half of guidance-rescale rows in the table-driven launch (DPM_TABLE_RESCALE, C ABI version 213): the real library's
DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_thresh_host.py.  With the flag every DPM_F_CFG_RESCALE
request that passes rescale_row_ok owns a row, from a group of one on, in runs of its own; without it the call is version
212's.  Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_host import FIELDS, HDR, N, POISON, ROW

RSC = L.TABLE_RESCALE
CFG = L.GUIDE["classifier-free"]
BASE_MODES = (1, 2, 5, 6, 9, 10, 13, 14, 33, 34, 37, 38, 41, 42, 45, 46)         # the valid modes of version 212
SCALES, PHIS = (1.5, 3.0, 7.5), (0.7, 1.0, 0.25)


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _div_ok(v):
    """div_invariant_ok of csrc/dpm_launch.hpp"""
    u = _bits(v)
    ex = (u >> 23) & 0xff
    return ex not in (0, 0xff) and (u & 0x7fffff) != 0x7fffff and 32 < ex < 222


def params_words(s):
    """the 20 words make_params (csrc/dpm_launch.hpp) writes for stage record s, in KParams' order"""
    one = np.float32(1.0)
    return [_bits(s.alpha_e), s.flags, _bits(s.sigma_e), s.model_type & 0xffffffff, _bits(s.cfg_scale), s.form, _bits(s.cg_scale),
            s.guidance, _bits(s.cx), _bits(s.c0), _bits(s.c1), _bits(s.c2)] + [_bits(s.k[j]) for j in range(5)] + [
            _bits(one / np.float32(s.alpha_e)), _bits(one / np.float32(s.sigma_e)),
            (1 if _div_ok(s.alpha_e) else 0) | (2 if _div_ok(s.sigma_e) else 0)]


class Call:
    """n_req well-formed classifier-free requests with CPU pointers (never dereferenced); kinds[r] = "rsc" (DPM_F_CFG_RESCALE,
    a phi and a guidance scale of its own) or "ode" (plain); forms rotate over LIN1 / TWO / MS3 / DENOISE for rescale rows and
    LIN1 / TWO / MS3 for plain ones; STORE_M and x_out2 alternate.  The table leaves room for both record sections."""

    def __init__(self, kinds, n=N, batch=1, dt=L.DTYPE_F16):
        R = self.R = len(kinds)
        self.st, self.bs = (L.Stage * R)(), (L.Buffers * R)()
        self.arena = np.zeros(64, dtype=np.uint8)
        p0 = (self.arena.ctypes.data + 63) // 64 * 64              # addresses only: spaced 2^20 bytes apart, 16-byte aligned
        for r, kind in enumerate(kinds):
            s, b = self.st[r], self.bs[r]
            rsc = kind == "rsc"
            forms = (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3) + ((L.FORM_DENOISE,) if rsc else ())
            s.index, s.form = r % 5, forms[r % len(forms)]
            s.flags = L.F_TO_X0 | (L.F_STORE_M if r % 2 else 0) | (L.F_CFG_RESCALE if rsc else 0)
            s.model_type, s.guidance = L.MODEL["noise"], CFG
            s.alpha_e, s.sigma_e = 0.75 + 0.001 * r, 0.5 - 0.001 * r
            s.cfg_scale = SCALES[r % 3]
            s.cg_scale = PHIS[(r // 3) % 3] if rsc else s.cfg_scale * s.sigma_e
            s.cx, s.c0, s.c1, s.c2 = 0.9, -0.1 - 0.01 * r, 0.05, 0.01
            for j in range(5):
                s.k[j] = 0.1 * (j + 1) + 0.001 * r
            p = [p0 + ((r * 8 + k) << 20) for k in range(8)]
            b.x, b.e0, b.e1, b.x_out, b.m_out = p[0], p[1], p[2], p[5], p[6]
            if s.form in (L.FORM_TWO, L.FORM_MS3):
                b.h1 = p[3]
            if s.form == L.FORM_MS3:
                b.h2 = p[4]
            if r % 4 != 3:
                b.x_out2 = p[7]
            b.n, b.batch = n * batch, batch
            b.state_dtype = b.eps_dtype = dt
        self.opts = L.LaunchOpts()
        self.opts.per_request_stages = 1
        self.bs[0].opts = C.pointer(self.opts)
        self.size = HDR + R * (ROW + L.TABLE_NOISE_BYTES + L.TABLE_BLEND_BYTES)
        self.table = np.full(self.size + 64 + 16, POISON, dtype=np.uint8)
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def run(self, mode):
        self.opts.table_mode = mode
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, None)
        return rc, L.lib.dpm_last_error().decode()

    def fill(self, mode=L.TABLE_FILL | RSC):
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
        """rows [first, first + len(members)) are those of `members`, in order: the 8 pointers, then make_params of the stage --
        its own cfg_scale and cg_scale among the 20 words"""
        members = list(members)
        ptr, words = self.rows(first, len(members))
        want = np.array([[getattr(self.bs[r], f) or 0 for f in FIELDS] for r in members], dtype=np.uint64)
        assert np.array_equal(ptr, want)
        assert words.tolist() == [params_words(self.st[r]) for r in members]


def test_abi_213_and_the_modes():
    assert L.lib.dpm_version() >= 213
    assert RSC == 128 and (L.TABLE_FILL, L.TABLE_LAUNCH, L.TABLE_NOISE, L.TABLE_THRESH, L.TABLE_BLEND) == (1, 2, 4, 8, 32)
    # no new record, no struct resized: the sizes of version 211
    assert [int(L.lib.dpm_sizeof(i)) for i in (7, 8, 9, 10, 11, 12, 13)] == [16, 144, 0, 32, 0, 48, 0]
    for flags in (0, 4, 8, 32, 4 | 8 | 32):
        assert L.table_bytes(20, flags | RSC) == L.table_bytes(20, flags)
    assert L.table_bytes(20, RSC) == HDR + 20 * ROW
    valid = set(BASE_MODES) | {m | RSC for m in BASE_MODES}
    for mode in list(range(-1, 70)) + list(range(126, 260)):
        if mode in valid or mode == 0:
            continue
        c = Call(["rsc"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)
    for flags in (0, 4, 8, 32, 4 | 8, 4 | 32, 8 | 32, 4 | 8 | 32):              # every valid FILL mode with bit 128 fills
        c = Call(["rsc"] * 20).fill(L.TABLE_FILL | RSC | flags)
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 20, 1], flags
        c.check_run(0, range(20))
        assert c.poison(HDR + 20 * ROW), "a rescale row has no record"


def test_rescale_groups_of_40_17_2_and_1_among_plain_rows():
    """four rescale groups (noise + TO_X0, v + TO_X0, noise eps-form, x_start) of 40, 17, 2 and 1 members interleaved with 20
    plain rows: a run each in the order the groups open, members in call order, ONE row counter, the header counts the runs"""
    keys = {"a": ("noise", True, 40), "b": ("v", True, 17), "c": ("noise", False, 2), "d": ("x_start", True, 1)}
    order = []
    left = {k: v[2] for k, v in keys.items()}
    left["ode"] = 20
    i = 0
    while any(left.values()):
        k = ("ode", "a", "b", "a", "c", "a", "d", "b")[i % 8]
        i += 1
        if left[k]:
            left[k] -= 1
            order.append(k)
    c = Call(["ode" if k == "ode" else "rsc" for k in order])
    for r, k in enumerate(order):
        if k != "ode":
            c.st[r].model_type = L.MODEL[keys[k][0]]
            if not keys[k][1]:
                c.st[r].flags &= ~L.F_TO_X0
    c.fill()
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(order), 5]
    first = 0
    for k in sorted(set(order), key=order.index):                   # the runs in the order their groups open
        members = [r for r, kk in enumerate(order) if kk == k]
        if k == "ode":
            ms3 = [r for r in members if c.st[r].form == L.FORM_MS3]
            assert len(members) == 20 and ms3
        c.check_run(first, members)
        first += len(members)
    assert first == len(order) and c.poison(HDR + first * ROW)
    rsc = [r for r, k in enumerate(order) if k == "a"]
    assert {c.st[r].form for r in rsc} == {L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3, L.FORM_DENOISE}       # the four forms share a run
    assert len({c.st[r].cfg_scale for r in rsc}) == 3 and len({c.st[r].cg_scale for r in rsc}) == 3 # ... so do scales and phis
    assert {bool(c.bs[r].x_out2) for r in rsc} == {True, False}


@pytest.mark.parametrize("R", [1, 2, 17])
@pytest.mark.parametrize("batch", [1, 3])
def test_a_group_of_one_owns_a_row(R, batch):
    c = Call(["rsc"] * R, n=8, batch=batch, dt=L.DTYPE_F32).fill()
    assert c.header()[2:] == [R, 1]
    c.check_run(0, range(R))
    assert c.poison(HDR + R * ROW)
    c = Call(["ode"] * 10 + ["rsc"]).fill()                        # ... beside a plain group too small for rows
    assert c.header()[2:] == [11, 1]
    c.check_run(0, [10])
    assert c.poison(HDR + ROW)


def _disqualify(c, r, what):
    s, b = c.st[r], c.bs[r]
    if what == "per_sample 7":
        b.n, b.batch = 56, 8
    elif what == "per_sample 12":
        b.n, b.batch = 24, 2
    elif what == "misaligned":
        b.h1 = b.x + 8
        s.form = L.FORM_TWO
    elif what == "misaligned x_out2":
        b.x_out2 = b.x_out + (1 << 19) + 8
    elif what == "separate xe":
        b.xe = b.x + (1 << 19)
    elif what == "phi 0":
        s.cg_scale = 0.0
    elif what == "phi 1.5":
        s.cg_scale = 1.5
    elif what == "thresholded":
        s.flags |= L.F_THRESH
    elif what == "unipc":
        s.form, b.h1 = L.FORM_UNIPC, b.x + (1 << 18)
        s.flags |= L.F_UNIPC_P2
    elif what == "ss3t":
        s.form, b.h1, b.h2 = L.FORM_SS3T, b.x + (1 << 18), b.x + (1 << 17)


# what dpm_stage_launch answers such a request today: (code, text), None = it is accepted and launched on its own
OUTSIDERS = {"per_sample 7": None, "per_sample 12": None, "misaligned": None, "misaligned x_out2": None, "separate xe": None,
             "ss3t": None,
             "phi 0": (L.ERR_ARG, "not in (0, 1]"), "phi 1.5": (L.ERR_ARG, "not in (0, 1]"),
             "thresholded": (L.ERR_UNSUPPORTED, "thresholding, mask blend or noise"),
             "unipc": (L.ERR_UNSUPPORTED, "DPM_FORM_UNIPC")}


@pytest.mark.parametrize("what", sorted(OUTSIDERS))
def test_a_flagged_request_that_fails_the_predicate_owns_no_row(what):
    c = Call(["rsc"] * 21)
    _disqualify(c, 7, what)
    # the code of the request's own dpm_stage_launch, decided before any HIP call (an accepted one is not launched here)
    if OUTSIDERS[what] is not None:
        lone = L.lib.dpm_stage_launch(C.byref(c.st[7]), C.byref(c.bs[7]), None)
        assert lone == OUTSIDERS[what][0] and OUTSIDERS[what][1] in L.lib.dpm_last_error().decode()
        before = c.table.copy()
        rc, msg = c.run(L.TABLE_FILL | RSC)
        assert rc == lone and OUTSIDERS[what][1] in msg, (rc, msg)      # the call reports it, as without the flag ...
        assert np.array_equal(c.table, before)                        # ... and writes nothing
        rc0, msg0 = c.run(L.TABLE_FILL)
        assert (rc0, msg0) == (rc, msg)
        return
    c.fill()
    others = [r for r in range(21) if r != 7]
    assert c.header()[2:] == [21, 1]
    c.check_run(0, others)
    assert c.poison(HDR + 20 * ROW)
    ref = Call(["rsc"] * 21).fill()                                # the others' rows: what they are without the outsider
    assert np.array_equal(c.rows(0, 20)[1], ref.rows(0, 21)[1][np.array(others)])


def test_a_row_of_other_n_batch_or_dtype_opens_its_own_run():
    c = Call(["rsc"] * 12)
    c.bs[3].n, c.bs[3].batch = 2 * N, 2                            # another n and batch
    c.bs[5].state_dtype = L.DTYPE_F32                              # another pair: fp32 state, fp16 outputs
    c.st[8].model_type = L.MODEL["v"]
    c.fill()
    assert c.header()[2:] == [12, 4]
    c.check_run(0, [r for r in range(12) if r not in (3, 5, 8)])
    c.check_run(9, [3])
    c.check_run(10, [5])
    c.check_run(11, [8])


def test_without_the_flag_every_call_is_version_212s():
    kinds = [("ode", "rsc")[r % 2] for r in range(40)]
    for mode in (L.TABLE_FILL, L.TABLE_FILL | L.TABLE_NOISE, L.TABLE_FILL | L.TABLE_THRESH | L.TABLE_BLEND):
        c = Call(kinds).fill(mode)
        ode = list(range(0, 40, 2))
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 40, 1]
        c.check_run(0, ode)
        assert c.poison(HDR + len(ode) * ROW), "a flagged request wrote a row without DPM_TABLE_RESCALE"
        was = c.bytes()[HDR:HDR + len(ode) * ROW].copy()           # ... and the plain rows are byte for byte those the flag leaves
        c.table[:] = POISON
        c.fill(mode | RSC)
        assert c.header()[2:] == [40, 2] and np.array_equal(c.bytes()[HDR:HDR + len(ode) * ROW], was)
        c.check_run(20, list(range(1, 40, 2)))
    # a request's own error keeps mode 0's text, and nothing is written
    c = Call(["rsc"] * 20)
    c.bs[11].e1 = None
    before = c.table.copy()
    rc, msg = c.run(L.TABLE_FILL | RSC)
    assert rc == L.ERR_ARG and "CFG needs e1" in msg and np.array_equal(c.table, before)
