"""The host half of two-condition rows in the table-driven launch (DPM_TABLE_PAIR, C ABI version 219): the real library's
DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_zstar_host.py.  With the flag every DPM_GUIDE_CFG2
request that passes pair_row_ok owns a row and a pair record behind the rows -- behind the noise, blend and APG records where
the call has those sections --, from a group of one on, in runs of its own, and such a request may carry x_out2 with the third
copy of x_out in dpm_buffers.thr_hint; without the flag the call is version 218's.  Nothing here launches a kernel, and FILL
calls no HIP function: every pointer is a CPU address that is never dereferenced, and the calls succeed on a machine without a
GPU."""
import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_apg_host import _bits, apg_offset
from test_table_host import HDR, N, POISON, ROW
from test_table_rescale_host import params_words
from test_table_zstar_host import MODES_215, ZCall

PR, ZST, APG = L.TABLE_PAIR, L.TABLE_ZSTAR, L.TABLE_APG
REC = 16
CFG2 = L.GUIDE["classifier-free-2"]
MODES_217 = tuple(MODES_215) + tuple(m | ZST for m in MODES_215)                # the 128 valid modes of version 217
ALL_FLAGS = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_RESCALE | APG | ZST
FORMS = (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3, L.FORM_DENOISE)
S2 = (0.75, -1.5, 2.5)
X_OUT2 = "stage_launch: DPM_GUIDE_CFG2 with x_out2 (the kernel has no second store)"
BOTH = ("stage_launch_multi: DPM_GUIDE_CFG2 in a DPM_TABLE_PAIR call needs x_out2 and the third copy (dpm_buffers.thr_hint) "
        "both set or both null")


def pair_offset(R, flags):
    """the documented offset of the pair section (include/dpm_hip.h, "Table mode")"""
    return apg_offset(R, flags) + (R * L.TABLE_APG_BYTES if flags & APG else 0)


class PCall(ZCall):
    """test_table_zstar_host.ZCall with a fifth kind, "pair": a DPM_GUIDE_CFG2 record -- s1 in cfg_scale, s2 in cg_scale, the
    third output in g; forms rotate over LIN1 / TWO / MS3 / DENOISE, STORE_M alternates, and three rows of four carry the two
    copies (x_out2 and, in thr_hint, the third).  The table leaves room for every record section."""

    def __init__(self, kinds, **kw):
        super().__init__(["ode" if k == "pair" else k for k in kinds], **kw)
        p0 = (self.arena.ctypes.data + 63) // 64 * 64
        for r, k in enumerate(kinds):
            if k != "pair":
                continue
            s, b = self.st[r], self.bs[r]
            s.guidance, s.form, s.cg_scale = CFG2, FORMS[r % 4], S2[r % 3]
            p = [p0 + ((r * 16 + j) << 20) for j in range(12)]
            b.h1 = p[3] if s.form in (L.FORM_TWO, L.FORM_MS3) else None
            b.h2 = p[4] if s.form == L.FORM_MS3 else None
            b.g = p[9]
            b.thr_hint = p[10] if b.x_out2 else None
        self.size += self.R * REC
        self.table = np.full(self.size + 64 + 16, POISON, dtype=np.uint8)
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def fill(self, mode=L.TABLE_FILL | PR):
        return super().fill(mode)

    def check_run(self, first, members):
        """ZCall's check of the rows and the APG records, then beside every row of a pair member its record -- g, then the
        third copy (thr_hint) -- and beside every other row a slot FILL did not touch"""
        members = list(members)
        super().check_run(first, members)
        if not self.mode & PR:
            return
        off = pair_offset(self.R, self.mode)
        for i, r in enumerate(members):
            raw = self.bytes()[off + (first + i) * REC:off + (first + i + 1) * REC].copy()
            if self.st[r].guidance != CFG2:
                assert bool((raw == POISON).all()), (r, "a record beside a row that is no pair row")
                continue
            assert [int(v) for v in raw.view(np.uint64)] == [self.bs[r].g or 0, self.bs[r].thr_hint or 0], r


def test_abi_219_the_constants_and_the_modes():
    assert L.lib.dpm_version() >= 219
    assert PR == 16384 and (L.TABLE_FILL, L.TABLE_LAUNCH, L.TABLE_NOISE, L.TABLE_THRESH, L.TABLE_BLEND, L.TABLE_RESCALE, APG, ZST) == (
        1, 2, 4, 8, 32, 128, 512, 4096)
    # (index 16 is pinned as unassigned since version 217, tests/test_table_zstar_host.py: the record takes the next even one)
    assert L.SIZEOF_TABLE_PAIR == 18 and L.TABLE_PAIR_BYTES == REC == int(L.lib.dpm_sizeof(L.SIZEOF_TABLE_PAIR))
    assert [int(L.lib.dpm_sizeof(i)) for i in (14, 15, 16, 17, 18, 19)] == [32, 0, 0, 0, 16, 0]
    for flags in sorted({m & ~3 for m in MODES_217}):
        assert L.table_bytes(20, flags | PR) == L.table_bytes(20, flags) + 20 * REC == pair_offset(20, flags) + 20 * REC, flags
    assert L.table_bytes(20, PR) == HDR + 20 * (ROW + REC)
    valid = set(MODES_217) | {m | PR for m in MODES_217}
    assert len(valid) == 256 and len(MODES_217) == 128
    for base in MODES_217:                                         # each previously valid mode, with and without 16384
        for mode in (base, base | PR):
            c = PCall(["pair"] * 3 + ["ode"] * 2)
            if mode & L.TABLE_FILL:
                for r in range(3):                                 # (without the flag a pair request carries no copy)
                    if not mode & PR:
                        c.bs[r].x_out2 = c.bs[r].thr_hint = None
                c.fill(mode)
                assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 5, 1 if mode & PR else 0], mode
    for mode in (16384, 16384 | 3, 32768 | 16384 | 1, 16384 | 8192 | 1, 16384 | 16 | 1, 16384 | 2048 | 2, 32768 | 1, 1 << 30):
        assert mode not in valid
        c = PCall(["pair"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg and "DPM_TABLE_PAIR" in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)


@pytest.mark.parametrize("R", [1, 2, 17])
@pytest.mark.parametrize("dt", [L.DTYPE_F16, L.DTYPE_F32, L.DTYPE_BF16])
def test_a_group_of_one_owns_a_row_and_a_record(R, dt):
    c = PCall(["pair"] * R, n=8, dt=dt).fill()
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
    c.check_run(0, range(R))
    assert c.poison(HDR + R * ROW, pair_offset(R, PR)) and c.poison(pair_offset(R, PR) + R * REC)


def test_the_row_is_8_pointers_and_20_words_and_the_record_two_pointers():
    """byte for byte: table_fill_rows writes the record as it is -- s1 in word 4, s2 in word 6, guidance 3 in word 7, x_out2 the
    eighth pointer -- and table_fill_pair writes (g, thr_hint) at the documented offset"""
    c = PCall(["pair"] * 8).fill()
    ptr, words = c.rows(0, 8)
    off = pair_offset(8, PR)
    assert off == HDR + 8 * ROW and ROW == 8 * 8 + 20 * 4
    for r in range(8):
        s, b = c.st[r], c.bs[r]
        assert [int(v) for v in ptr[r]] == [b.x or 0, b.e0 or 0, b.e1 or 0, b.h1 or 0, b.h2 or 0, b.x_out or 0, b.m_out or 0, b.x_out2 or 0]
        assert words[r].tolist() == params_words(s) and len(words[r]) == 20
        assert int(words[r, 4]) == _bits(s.cfg_scale) and int(words[r, 6]) == _bits(s.cg_scale) and int(words[r, 7]) == CFG2
        rec = c.bytes()[off + r * REC:off + (r + 1) * REC].copy().view(np.uint64)
        assert [int(v) for v in rec] == [b.g, b.thr_hint or 0]
    assert {bool(c.bs[r].x_out2) for r in range(8)} == {True, False}               # rows with and without the copies,
    assert {c.st[r].form for r in range(8)} == set(FORMS)                          # the four forms,
    assert len({c.st[r].cg_scale for r in range(8)}) == 3 and len({c.st[r].cfg_scale for r in range(8)}) == 3   # both scales
    assert {bool(c.st[r].flags & L.F_STORE_M) for r in range(8)} == {True, False}  # and DPM_F_STORE_M share ONE run


def test_the_record_sits_behind_the_noise_blend_and_apg_sections_of_a_call_with_every_flag():
    c = PCall(["pair"] * 6).fill(L.TABLE_FILL | PR | ALL_FLAGS)
    R = 6
    off = pair_offset(R, PR | ALL_FLAGS)
    assert off == HDR + R * (ROW + L.TABLE_NOISE_BYTES + L.TABLE_BLEND_BYTES + L.TABLE_APG_BYTES)
    assert off + R * REC == L.table_bytes(R, PR | ALL_FLAGS)
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
    c.check_run(0, range(R))
    assert c.poison(HDR + R * ROW, off) and c.poison(off + R * REC)               # the other sections: untouched


def test_pair_requests_next_to_plain_zstar_and_apg_requests_each_in_its_own_run():
    """a CFG2 group among 20 plain, 5 CFG-Zero* and 6 APG requests under all flags: a run each in the order the groups open,
    members in call order, ONE row counter, a header run count that includes the pair run, and the record slots of the other
    kinds' rows untouched"""
    order, left, i = [], {"ode": 20, "pair": 9, "zst": 5, "apg": 6}, 0
    while any(left.values()):
        k = ("ode", "pair", "zst", "ode", "apg", "pair")[i % 6]
        i += 1
        if left[k]:
            left[k] -= 1
            order.append(k)
    c = PCall(order).fill(L.TABLE_FILL | PR | ALL_FLAGS)
    R = len(order)
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 4]
    first = 0
    for k in sorted(set(order), key=order.index):
        members = [r for r, kk in enumerate(order) if kk == k]
        c.check_run(first, members)
        first += len(members)
    assert first == R and c.poison(HDR + R * ROW, apg_offset(R, ALL_FLAGS))
    # a pair request of another model type or prologue opens a run of its own (het_same_group's keys)
    c = PCall(["pair"] * 6)
    c.st[2].model_type = L.MODEL["v"]
    c.st[4].flags &= ~L.F_TO_X0
    c.fill()
    assert c.header()[2:] == [6, 3]
    c.check_run(0, [0, 1, 3, 5])
    c.check_run(4, [2])
    c.check_run(5, [4])


def _disqualify(c, r, what):
    s, b = c.st[r], c.bs[r]
    if what == "n % 8":
        b.n = N + 4
    elif what == "misaligned":
        b.e1 = b.e1 + 8
    elif what == "misaligned g":
        b.g = b.g + 8
    elif what == "separate xe":
        b.xe = b.x + (1 << 19)
    elif what == "ss3t":
        s.form, b.h1, b.h2 = L.FORM_SS3T, b.x + (1 << 18), b.x + (1 << 17)
    elif what == "multi_fuse off":
        pass


@pytest.mark.parametrize("what", ["n % 8", "misaligned", "misaligned g", "separate xe", "ss3t"])
def test_a_request_without_copies_that_fails_the_predicate_goes_alone(what):
    """... as today: no row, no error, the others' rows what they are without it"""
    c = PCall(["pair"] * 9)
    c.bs[5].x_out2 = c.bs[5].thr_hint = None
    _disqualify(c, 5, what)
    c.fill()
    others = [r for r in range(9) if r != 5]
    assert c.header()[2:] == [9, 1]
    c.check_run(0, others)
    assert c.poison(HDR + 8 * ROW, pair_offset(9, PR)) and c.poison(pair_offset(9, PR) + 8 * REC)


def test_every_new_refusal_comes_before_anything_is_written():
    # one copy without the other
    for which in ("x_out2", "thr_hint"):
        c = PCall(["pair"] * 9)
        assert c.bs[4].x_out2 and c.bs[4].thr_hint
        setattr(c.bs[4], which, None)
        before = c.table.copy()
        for mode in (L.TABLE_FILL | PR, L.TABLE_LAUNCH | PR):
            rc, msg = c.run(mode)
            assert (rc, msg) == (L.ERR_ARG, BOTH), (which, mode, rc, msg)
            assert np.array_equal(c.table, before)
    # copies on a request without a row: the lone kernel's refusal, for the whole call
    for what in ("n % 8", "misaligned", "misaligned g", "separate xe", "ss3t"):
        c = PCall(["pair"] * 9)
        assert c.bs[4].x_out2
        _disqualify(c, 4, what)
        before = c.table.copy()
        rc, msg = c.run(L.TABLE_FILL | PR)
        assert (rc, msg) == (L.ERR_UNSUPPORTED, X_OUT2), (what, rc, msg)
        assert np.array_equal(c.table, before)
    for which, ptr in (("x_out2", 8), ("thr_hint", 8)):            # a misaligned copy is no row either
        c = PCall(["pair"] * 9)
        setattr(c.bs[4], which, getattr(c.bs[4], which) + ptr)
        before = c.table.copy()
        rc, msg = c.run(L.TABLE_FILL | PR)
        assert (rc, msg) == (L.ERR_UNSUPPORTED, X_OUT2) and np.array_equal(c.table, before)
    # x_out2 without the flag keeps today's text, in every mode
    for mode in (L.TABLE_FILL, L.TABLE_FILL | ALL_FLAGS, L.TABLE_LAUNCH | ZST):
        c = PCall(["pair"] * 9)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert (rc, msg) == (L.ERR_UNSUPPORTED, X_OUT2) and np.array_equal(c.table, before)
    # the guidance's own checks keep their texts under the flag
    c = PCall(["pair"] * 9)
    c.st[3].cg_scale = float("inf")
    rc, msg = c.run(L.TABLE_FILL | PR)
    assert rc == L.ERR_ARG and "both must be finite" in msg
    c = PCall(["pair"] * 9)
    c.bs[3].g = None
    rc, msg = c.run(L.TABLE_FILL | PR)
    assert rc == L.ERR_ARG and "DPM_GUIDE_CFG2 needs e1 and g" in msg


def test_without_the_flag_every_call_is_version_218s():
    kinds = [("ode", "pair")[r % 2] for r in range(40)]
    ode = list(range(0, 40, 2))
    for mode in (L.TABLE_FILL, L.TABLE_FILL | L.TABLE_NOISE, L.TABLE_FILL | ALL_FLAGS):
        c = PCall(kinds)
        for r in range(1, 40, 2):
            c.bs[r].x_out2 = None                                  # (refused without the flag); thr_hint stays: ignored as today
        c.fill(mode)
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 40, 1]
        c.check_run(0, ode)
        assert c.poison(HDR + len(ode) * ROW), "a two-condition request wrote a row without DPM_TABLE_PAIR"
        was = c.bytes()[HDR:HDR + len(ode) * ROW].copy()           # ... and the plain rows are byte for byte those the flag leaves
        for r in range(1, 40, 2):
            c.bs[r].thr_hint = None
        c.table[:] = POISON
        c.fill(mode | PR)
        assert c.header()[2:] == [40, 2] and np.array_equal(c.bytes()[HDR:HDR + len(ode) * ROW], was)
        c.check_run(20, list(range(1, 40, 2)))
