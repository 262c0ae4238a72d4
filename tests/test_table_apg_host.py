"""The host half of adaptive-projected-guidance rows in the table-driven launch (DPM_TABLE_APG, C ABI version 215): the real
library's DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_rescale_host.py.  With the flag every
DPM_F_CFG_APG request that passes apg_row_ok owns a row and an APG record behind the rows -- behind the noise and the blend
records where the call has those sections --, from a group of one on, in runs of its own, and the running average of every
such request is dpm_buffers.thr_hint; without the flag the call is version 214's.  Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_host import FIELDS, HDR, N, POISON, ROW
from test_table_rescale_host import BASE_MODES, params_words

APG, RSC = L.TABLE_APG, L.TABLE_RESCALE
REC = 32
CFG = L.GUIDE["classifier-free"]
MODES_214 = tuple(BASE_MODES) + tuple(m | RSC for m in BASE_MODES)              # the valid modes of version 214
SCALES = (1.5, 3.0, 7.5)
ETAS, RS, BETAS = (0.0, 0.5, 1.0), (0.0, 1e-3, 1e6), (0.0, -0.5, 0.25)


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def apg_offset(R, flags):
    """the documented offset of the APG section (include/dpm_hip.h, "Table mode")"""
    return HDR + R * ROW + (R * L.TABLE_NOISE_BYTES if flags & L.TABLE_NOISE else 0) + (R * L.TABLE_BLEND_BYTES if flags & L.TABLE_BLEND else 0)


class Call:
    """n_req well-formed classifier-free requests with CPU pointers (never dereferenced); kinds[r] = "apg" (DPM_F_CFG_APG with
    eta, r, beta and a guidance scale of its own, the running average in thr_hint where beta != 0), "rsc" (DPM_F_CFG_RESCALE)
    or "ode" (plain); forms rotate over LIN1 / TWO / MS3 / DENOISE for the per-sample kinds and LIN1 / TWO / MS3 for plain
    ones; STORE_M and x_out2 alternate.  The table leaves room for all three record sections."""

    def __init__(self, kinds, n=N, batch=1, dt=L.DTYPE_F16):
        R = self.R = len(kinds)
        self.st, self.bs = (L.Stage * R)(), (L.Buffers * R)()
        self.arena = np.zeros(64, dtype=np.uint8)
        p0 = (self.arena.ctypes.data + 63) // 64 * 64              # addresses only: spaced 2^20 bytes apart, 16-byte aligned
        for r, kind in enumerate(kinds):
            s, b = self.st[r], self.bs[r]
            apg, rsc = kind == "apg", kind == "rsc"
            forms = (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3) + ((L.FORM_DENOISE,) if apg or rsc else ())
            s.index, s.form = r % 5, forms[r % len(forms)]
            s.flags = L.F_TO_X0 | (L.F_STORE_M if r % 2 else 0) | (L.F_CFG_APG if apg else 0) | (L.F_CFG_RESCALE if rsc else 0)
            s.model_type, s.guidance = L.MODEL["noise"], CFG
            s.alpha_e, s.sigma_e = 0.75 + 0.001 * r, 0.5 - 0.001 * r
            s.cfg_scale = SCALES[r % 3]
            s.cg_scale = s.cfg_scale * s.sigma_e
            if rsc:
                s.cg_scale = 0.7
            s.cx, s.c0, s.c1, s.c2 = 0.9, -0.1 - 0.01 * r, 0.05, 0.01
            for j in range(5):
                s.k[j] = 0.1 * (j + 1) + 0.001 * r
            p = [p0 + ((r * 16 + k) << 20) for k in range(9)]
            b.x, b.e0, b.e1, b.x_out, b.m_out = p[0], p[1], p[2], p[5], p[6]
            if apg:
                s.cg_scale, s.thr_ratio, s.thr_max = ETAS[r % 3], RS[(r // 3) % 3], BETAS[(r // 2) % 3]
                if s.thr_max != 0:
                    b.thr_hint = p[8]
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
        self.size = HDR + R * (ROW + L.TABLE_NOISE_BYTES + L.TABLE_BLEND_BYTES + REC)
        self.table = np.full(self.size + 64 + 16, POISON, dtype=np.uint8)
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def run(self, mode):
        self.opts.table_mode = mode
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, None)
        return rc, L.lib.dpm_last_error().decode()

    def fill(self, mode=L.TABLE_FILL | APG):
        self.mode = mode
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
        """rows [first, first + len(members)) are those of `members`, in order: the 8 pointers, then make_params of the stage;
        beside every row of an APG member its record, word for word -- the average (thr_hint; null when beta == 0), the bits of
        eta, r and beta, three zero words -- and beside every other row a slot FILL did not touch"""
        members = list(members)
        ptr, words = self.rows(first, len(members))
        want = np.array([[getattr(self.bs[r], f) or 0 for f in FIELDS] for r in members], dtype=np.uint64)
        assert np.array_equal(ptr, want)
        assert words.tolist() == [params_words(self.st[r]) for r in members]
        if not self.mode & APG:
            return
        off = apg_offset(self.R, self.mode)
        for i, r in enumerate(members):
            raw = self.bytes()[off + (first + i) * REC:off + (first + i + 1) * REC].copy()
            s, b = self.st[r], self.bs[r]
            if not s.flags & L.F_CFG_APG:
                assert bool((raw == POISON).all()), (r, "a record beside a row that is no APG row")
                continue
            avg = (b.thr_hint or 0) if s.thr_max != 0 else 0
            assert int(raw[:8].view(np.uint64)[0]) == avg, (r, hex(avg))
            assert [int(v) for v in raw[8:].view(np.uint32)] == [_bits(s.cg_scale), _bits(s.thr_ratio), _bits(s.thr_max), 0, 0, 0], r


def test_abi_215_the_constants_and_the_modes():
    assert L.lib.dpm_version() >= 215
    assert APG == 512 and (L.TABLE_FILL, L.TABLE_LAUNCH, L.TABLE_NOISE, L.TABLE_THRESH, L.TABLE_BLEND, RSC) == (1, 2, 4, 8, 32, 128)
    assert L.SIZEOF_TABLE_APG == 14 and L.TABLE_APG_BYTES == REC
    assert [int(L.lib.dpm_sizeof(i)) for i in (7, 8, 9, 10, 11, 12, 13, 14, 15)] == [16, 144, 0, 32, 0, 48, 0, 32, 0]
    for flags in (0, 4, 8, 32, 128, 4 | 32, 4 | 8 | 32 | 128):
        assert L.table_bytes(20, flags | APG) == L.table_bytes(20, flags) + 20 * REC, flags
        assert L.table_bytes(20, flags | APG) == apg_offset(20, flags) + 20 * REC
    assert L.table_bytes(20, APG) == HDR + 20 * (ROW + REC)
    valid = set(MODES_214) | {m | APG for m in MODES_214}
    assert len(valid) == 64
    for mode in list(range(250, 520)) + list(range(760, 1030)) + [1024 | 1, 2048 | 513, 1 << 30]:
        if mode in valid:
            continue                                               # (modes below 260: tests/test_table_rescale_host.py)
        c = Call(["apg"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)
    for mode in (256 | 1, 256 | 2, 512 | 256 | 1, 512 | 256 | 128 | 2, 512 | 16 | 1, 512 | 64 | 2, 512, 512 | 3):
        assert mode not in valid                                   # bit 256 stays unassigned, like 16 and 64
    for base in MODES_214:                                         # every valid FILL mode with bit 512 fills
        if not base & L.TABLE_FILL:
            continue
        c = Call(["apg"] * 20).fill(base | APG)
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 20, 1], base
        c.check_run(0, range(20))
        off = apg_offset(20, base)
        assert c.poison(HDR + 20 * ROW, off) and c.poison(off + 20 * REC), base     # nothing but the rows and their records


def test_the_record_sits_behind_the_noise_and_the_blend_sections():
    for flags, off in ((0, HDR + 20 * ROW), (L.TABLE_NOISE, HDR + 20 * (ROW + 32)), (L.TABLE_BLEND, HDR + 20 * (ROW + 48)),
                       (L.TABLE_NOISE | L.TABLE_BLEND, HDR + 20 * (ROW + 32 + 48)), (L.TABLE_THRESH | RSC, HDR + 20 * ROW)):
        assert apg_offset(20, flags) == off
        c = Call(["apg"] * 20).fill(L.TABLE_FILL | APG | flags)
        c.check_run(0, range(20))
        recs = c.bytes()[off:off + 20 * REC].reshape(20, REC)
        assert not bool((recs == POISON).all(axis=1).any())
        # pointer, eta, r, beta, three zeros -- every combination of the three appears, with and without a momentum
        assert {bool(int(r[:8].view(np.uint64)[0])) for r in recs} == {True, False}
        for i, r in enumerate(recs):
            assert bool(int(r[:8].view(np.uint64)[0])) == (c.st[i].thr_max != 0)
            assert int(r[:8].view(np.uint64)[0]) in (0, c.bs[i].thr_hint)


def test_poison_outside_the_groups_record_slots_survives():
    kinds = [("ode", "apg", "rsc")[r % 3] for r in range(60)]
    c = Call(kinds).fill(L.TABLE_FILL | APG | RSC)
    ode, apg, rsc = ([r for r in range(60) if kinds[r] == k] for k in ("ode", "apg", "rsc"))
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 60, 3]
    c.check_run(0, ode)
    c.check_run(20, apg)
    c.check_run(40, rsc)
    off = apg_offset(60, APG | RSC)
    assert c.poison(off, off + 20 * REC) and c.poison(off + 40 * REC)            # records 20..39 and nothing else


def test_apg_groups_of_40_17_2_and_1_among_plain_and_rescale_rows():
    """four APG groups (noise, v, x_start, score networks) of 40, 17, 2 and 1 members interleaved with 20 plain and 5 rescale
    rows: a run each in the order the groups open, members in call order, ONE row counter, the header counts the runs"""
    keys = {"a": ("noise", 40), "b": ("v", 17), "c": ("x_start", 2), "d": ("score", 1)}
    order = []
    left = {k: v[1] for k, v in keys.items()}
    left["ode"], left["rsc"] = 20, 5
    i = 0
    while any(left.values()):
        k = ("ode", "a", "b", "a", "c", "rsc", "a", "d", "b")[i % 9]
        i += 1
        if left[k]:
            left[k] -= 1
            order.append(k)
    c = Call([k if k in ("ode", "rsc") else "apg" for k in order])
    for r, k in enumerate(order):
        if k in keys:
            c.st[r].model_type = L.MODEL[keys[k][0]]
    c.fill(L.TABLE_FILL | APG | RSC)
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(order), 6]
    first = 0
    for k in sorted(set(order), key=order.index):                   # the runs in the order their groups open
        members = [r for r, kk in enumerate(order) if kk == k]
        c.check_run(first, members)
        first += len(members)
    assert first == len(order) and c.poison(HDR + first * ROW, apg_offset(len(order), APG))
    a = [r for r, k in enumerate(order) if k == "a"]
    assert {c.st[r].form for r in a} == {L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3, L.FORM_DENOISE}         # the four forms share a run
    assert len({c.st[r].cfg_scale for r in a}) == 3 and len({c.st[r].cg_scale for r in a}) == 3     # ... so do scales and etas,
    assert len({c.st[r].thr_ratio for r in a}) == 3 and len({c.st[r].thr_max for r in a}) == 3     # thresholds and momenta
    assert {bool(c.bs[r].x_out2) for r in a} == {True, False}


@pytest.mark.parametrize("R", [1, 2, 17])
@pytest.mark.parametrize("batch", [1, 3])
def test_a_group_of_one_owns_a_row(R, batch):
    c = Call(["apg"] * R, n=8, batch=batch, dt=L.DTYPE_F32).fill()
    assert c.header()[2:] == [R, 1]
    c.check_run(0, range(R))
    assert c.poison(HDR + R * ROW, apg_offset(R, APG)) and c.poison(apg_offset(R, APG) + R * REC)
    c = Call(["ode"] * 10 + ["apg"]).fill()                        # ... beside a plain group too small for rows
    assert c.header()[2:] == [11, 1]
    c.check_run(0, [10])
    assert c.poison(HDR + ROW, apg_offset(11, APG))


MOMENTUM_0 = "stage_launch_multi: table_mode with a DPM_F_CFG_APG momentum in st[0] (bs[0].workspace is the table)"


def test_a_momentum_in_request_0_needs_the_flag():
    c = Call(["apg"] * 4)
    c.st[0].thr_max, c.bs[0].thr_hint = -0.5, c.bs[0].x + (9 << 20)
    for mode in (L.TABLE_FILL, L.TABLE_LAUNCH, L.TABLE_FILL | RSC, L.TABLE_LAUNCH | L.TABLE_NOISE):
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and msg == MOMENTUM_0, (mode, rc, msg)     # version 214's refusal, word for word
        assert np.array_equal(c.table, before)
    c.fill(L.TABLE_FILL | APG)                                     # with the flag the average is thr_hint: accepted
    assert c.header()[2:] == [4, 1]
    c.check_run(0, range(4))


def test_a_momentum_without_thr_hint_is_an_argument_error():
    for r in (0, 5):
        c = Call(["apg"] * 8)
        c.st[r].thr_max, c.bs[r].thr_hint = -0.5, None
        if r:
            c.bs[r].workspace = c.bs[r].x + (9 << 20)              # (workspace is not read for it in such a call)
        before = c.table.copy()
        rc, msg = c.run(L.TABLE_FILL | APG)
        assert rc == L.ERR_ARG and "running average in dpm_buffers.thr_hint" in msg, (rc, msg)
        assert np.array_equal(c.table, before)
        rc, msg = c.run(L.TABLE_LAUNCH | APG)                      # LAUNCH checks first too: nothing launched
        assert rc == L.ERR_ARG and "running average in dpm_buffers.thr_hint" in msg, (rc, msg)
    c = Call(["apg"] * 8)                                          # without the flag at r > 0: workspace, version 214's text
    c.st[5].thr_max, c.bs[5].workspace = -0.5, None
    rc, msg = c.run(L.TABLE_FILL)
    assert rc == L.ERR_ARG and "running average in dpm_buffers.workspace" in msg, (rc, msg)


def _disqualify(c, r, what):
    s, b = c.st[r], c.bs[r]
    if what == "per_sample 12":
        b.n, b.batch = 24, 2
    elif what == "per_sample 7":
        b.n, b.batch = 56, 8
    elif what == "average misaligned by 4":
        s.thr_max, b.thr_hint = -0.5, b.x + (9 << 20) + 4
    elif what == "misaligned":
        b.h1 = b.x + 8
        s.form = L.FORM_TWO
    elif what == "misaligned x_out2":
        b.x_out2 = b.x_out + (1 << 19) + 8
    elif what == "separate xe":
        b.xe = b.x + (1 << 19)
    elif what == "ss3t":
        s.form, b.h1, b.h2 = L.FORM_SS3T, b.x + (1 << 18), b.x + (1 << 17)
    elif what == "eta 1.5":
        s.cg_scale = 1.5
    elif what == "beta 1":
        s.thr_max, b.thr_hint = 1.0, b.x + (9 << 20)
    elif what == "thresholded":
        s.flags |= L.F_THRESH
    elif what == "rescale too":
        s.flags |= L.F_CFG_RESCALE
    elif what == "no TO_X0":
        s.flags &= ~L.F_TO_X0
    elif what == "unipc":
        s.form, b.h1 = L.FORM_UNIPC, b.x + (1 << 18)
        s.flags |= L.F_UNIPC_P2


# what the call answers such a request: (code, text), None = it is accepted and goes as its own launch, which still projects
OUTSIDERS = {"per_sample 12": None, "per_sample 7": None, "average misaligned by 4": None, "misaligned": None,
             "misaligned x_out2": None, "separate xe": None, "ss3t": None,
             "eta 1.5": (L.ERR_ARG, "not in [0, 1]"), "beta 1": (L.ERR_ARG, "not in (-1, 1)"),
             "thresholded": (L.ERR_UNSUPPORTED, "guidance rescale, thresholding, mask blend or noise"),
             "rescale too": (L.ERR_UNSUPPORTED, "guidance rescale, thresholding, mask blend or noise"),
             "no TO_X0": (L.ERR_UNSUPPORTED, "without DPM_F_TO_X0"),
             "unipc": (L.ERR_UNSUPPORTED, "DPM_FORM_UNIPC")}


@pytest.mark.parametrize("what", sorted(OUTSIDERS))
def test_a_flagged_request_that_fails_the_predicate_owns_no_row(what):
    c = Call(["apg"] * 21)
    _disqualify(c, 7, what)
    if OUTSIDERS[what] is not None:
        before = c.table.copy()
        rc, msg = c.run(L.TABLE_FILL | APG)
        assert rc == OUTSIDERS[what][0] and OUTSIDERS[what][1] in msg, (rc, msg)      # the call reports it ...
        assert np.array_equal(c.table, before)                        # ... and writes nothing
        return
    c.fill()
    others = [r for r in range(21) if r != 7]
    assert c.header()[2:] == [21, 1]
    c.check_run(0, others)
    off = apg_offset(21, APG)
    assert c.poison(HDR + 20 * ROW, off) and c.poison(off + 20 * REC)
    ref = Call(["apg"] * 21).fill()                                # the others' rows: what they are without the outsider
    assert np.array_equal(c.rows(0, 20)[1], ref.rows(0, 21)[1][np.array(others)])


def test_a_row_of_other_n_batch_or_dtype_opens_its_own_run():
    c = Call(["apg"] * 12)
    c.bs[3].n, c.bs[3].batch = 2 * N, 2                            # another n and batch
    c.bs[5].state_dtype = L.DTYPE_F32                              # another pair: fp32 state, fp16 outputs
    c.st[8].model_type = L.MODEL["v"]
    c.fill()
    assert c.header()[2:] == [12, 4]
    c.check_run(0, [r for r in range(12) if r not in (3, 5, 8)])
    c.check_run(9, [3])
    c.check_run(10, [5])
    c.check_run(11, [8])


def test_without_the_flag_every_call_is_version_214s():
    kinds = [("ode", "apg")[r % 2] for r in range(40)]
    for r0 in (0,):
        for mode in (L.TABLE_FILL, L.TABLE_FILL | L.TABLE_NOISE, L.TABLE_FILL | L.TABLE_THRESH | L.TABLE_BLEND | RSC):
            c = Call(kinds)
            for r in range(1, 40, 2):                              # (version 214: the average of a request at r > 0 is workspace)
                c.bs[r].workspace, c.bs[r].thr_hint = c.bs[r].thr_hint, None
            c.fill(mode)
            ode = list(range(0, 40, 2))
            assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 40, 1]
            c.check_run(0, ode)
            assert c.poison(HDR + len(ode) * ROW), "a flagged request wrote a row or a record without DPM_TABLE_APG"
            was = c.bytes()[HDR:HDR + len(ode) * ROW].copy()       # ... and the plain rows are byte for byte those the flag leaves
            for r in range(1, 40, 2):
                c.bs[r].workspace, c.bs[r].thr_hint = None, c.bs[r].workspace
            c.table[:] = POISON
            c.fill(mode | APG)
            assert c.header()[2:] == [40, 2] and np.array_equal(c.bytes()[HDR:HDR + len(ode) * ROW], was)
            c.check_run(20, list(range(1, 40, 2)))
    # a request's own error keeps mode 0's text, and nothing is written
    c = Call(["apg"] * 20)
    c.bs[11].e1 = None
    before = c.table.copy()
    rc, msg = c.run(L.TABLE_FILL | APG)
    assert rc == L.ERR_ARG and "CFG needs e1" in msg and np.array_equal(c.table, before)
