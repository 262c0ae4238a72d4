"""The host half of Perp-Neg rows in the table-driven launch (DPM_TABLE_PERP, C ABI version 221): the real library's
DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_pair_host.py.  With the flag every DPM_F_CFG2_PERP request
that passes perp_row_ok owns a row and a pair record -- in the pair records' section, which is present under DPM_TABLE_PAIR or
DPM_TABLE_PERP or both --, from a group of one on, in runs of its own, and such a request may carry x_out2 with the third copy of
x_out in dpm_buffers.thr_hint; a flagged request never owns a two-condition row; without the flag the call is version 220's.
Nothing here launches a kernel, and FILL calls no HIP function: every pointer is a CPU address that is never dereferenced, and the
calls succeed on a machine without a GPU."""
import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_apg_host import _bits
from test_table_host import HDR, N, POISON, ROW
from test_table_pair_host import ALL_FLAGS, BOTH, CFG2, MODES_217, REC, X_OUT2, PCall, _disqualify, pair_offset

PP, PR = L.TABLE_PERP, L.TABLE_PAIR
PERP = L.F_CFG2_PERP
MODES_219 = tuple(MODES_217) + tuple(m | PR for m in MODES_217)                 # the 256 valid modes of version 219
BOTH_PP = BOTH.replace("DPM_TABLE_PAIR", "DPM_TABLE_PERP")
NO_ROWS = "stage_launch_multi: DPM_F_CFG2_PERP in a table-mode call (the table's rows have no per-sample pass)"


class PerpCall(PCall):
    """test_table_pair_host.PCall with a sixth kind, "perp": a "pair" record with DPM_F_CFG2_PERP -- s in cfg_scale, w in
    cg_scale, the negative output in g; forms, STORE_M, scales and copies rotate as the pair kind's do"""

    def __init__(self, kinds, **kw):
        super().__init__(["pair" if k == "perp" else k for k in kinds], **kw)
        for r, k in enumerate(kinds):
            if k == "perp":
                self.st[r].flags |= PERP

    def fill(self, mode=L.TABLE_FILL | PP):
        return super().fill(mode)

    def check_run(self, first, members):
        """PCall's check of the rows (and, under DPM_TABLE_PAIR, of the pair rows' records); under DPM_TABLE_PERP beside every
        row of a flagged member its record -- g, then the third copy -- and, in a call without DPM_TABLE_PAIR, beside every
        other row a slot FILL did not touch"""
        members = list(members)
        mode = self.mode
        super().check_run(first, members)
        if not mode & PP:
            return
        off = pair_offset(self.R, mode)
        for i, r in enumerate(members):
            raw = self.bytes()[off + (first + i) * REC:off + (first + i + 1) * REC].copy()
            if self.st[r].flags & PERP:
                assert [int(v) for v in raw.view(np.uint64)] == [self.bs[r].g or 0, self.bs[r].thr_hint or 0], r
            elif not (mode & PR and self.st[r].guidance == CFG2):
                assert bool((raw == POISON).all()), (r, "a record beside a row that is neither a Perp-Neg nor a pair row")


def test_abi_221_the_constants_and_the_modes():
    assert L.lib.dpm_version() >= 221 and PP == 65536 and PR == 16384 and len(L.SYMBOLS) == 62
    assert [int(L.lib.dpm_sizeof(i)) for i in (17, 18, 19, 20, 21)] == [0, 16, 0, 0, 0]          # no new dpm_sizeof index
    # the pair section is present under either flag, once; without the new bit table_bytes is what it was
    for flags in sorted({m & ~3 for m in MODES_217}):
        base = L.table_bytes(20, flags)
        assert L.table_bytes(20, flags | PR) == base + 20 * REC
        assert L.table_bytes(20, flags | PP) == base + 20 * REC == pair_offset(20, flags | PP) + 20 * REC
        assert L.table_bytes(20, flags | PR | PP) == base + 20 * REC
    assert L.table_bytes(20, PP) == HDR + 20 * (ROW + REC)
    valid = set(MODES_219) | {m | PP for m in MODES_219}
    assert len(valid) == 512 and len(MODES_219) == 256
    for base in MODES_219:                                         # each previously valid mode, with and without 65536
        for mode in (base, base | PP):
            c = PerpCall(["perp"] * 3 + ["ode"] * 2)
            for r in range(3):
                if not mode & PP:
                    c.st[r].flags &= ~PERP                         # (without the flag a flagged request is refused: below)
                if not mode & (PP | PR):
                    c.bs[r].x_out2 = c.bs[r].thr_hint = None
            if mode & L.TABLE_FILL:
                c.fill(mode)
                assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 5, 1 if mode & (PP | PR) else 0], mode
    for mode in (65536, 65536 | 3, 65536 | 32768 | 1, 32768 | 1, 32768 | 16384 | 1, 65536 | 8192 | 1, 65536 | 16 | 2, 131072 | 1,
                 131072 | 65536 | 1, 65536 | 16384 | 32768 | 2, 1 << 30):
        assert mode not in valid
        c = PerpCall(["perp"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg and "DPM_TABLE_PAIR / DPM_TABLE_PERP)" in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)


@pytest.mark.parametrize("R", [1, 2, 17])
@pytest.mark.parametrize("dt", [L.DTYPE_F16, L.DTYPE_F32, L.DTYPE_BF16])
def test_a_group_of_one_owns_a_row_and_a_record(R, dt):
    c = PerpCall(["perp"] * R, n=8, dt=dt).fill()
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
    c.check_run(0, range(R))
    assert c.poison(HDR + R * ROW, pair_offset(R, PP)) and c.poison(pair_offset(R, PP) + R * REC)
    c = PerpCall(["perp"] * R, n=16, batch=3, dt=dt).fill()        # three samples per row
    assert c.header()[2:] == [R, 1]
    c.check_run(0, range(R))


def test_the_row_carries_the_flag_and_the_record_is_a_pair_record():
    c = PerpCall(["perp"] * 8).fill()
    ptr, words = c.rows(0, 8)
    off = pair_offset(8, PP)
    assert off == HDR + 8 * ROW
    for r in range(8):
        s, b = c.st[r], c.bs[r]
        assert int(words[r, 4]) == _bits(s.cfg_scale) and int(words[r, 6]) == _bits(s.cg_scale) and int(words[r, 7]) == CFG2
        assert PERP in [int(v) & PERP for v in words[r]]                         # the flags word carries DPM_F_CFG2_PERP
        assert int(ptr[r, 7]) == (b.x_out2 or 0)
        rec = c.bytes()[off + r * REC:off + (r + 1) * REC].copy().view(np.uint64)
        assert [int(v) for v in rec] == [b.g, b.thr_hint or 0]
    assert {bool(c.bs[r].x_out2) for r in range(8)} == {True, False}               # rows with and without the copies,
    assert len({c.st[r].form for r in range(8)}) == 4                              # the four forms,
    assert len({c.st[r].cg_scale for r in range(8)}) == 3 and len({c.st[r].cfg_scale for r in range(8)}) == 3   # both scales
    assert {bool(c.st[r].flags & L.F_STORE_M) for r in range(8)} == {True, False}  # and DPM_F_STORE_M share ONE run
    # the same requests under every flag: the section sits behind the noise, blend and APG records
    c = PerpCall(["perp"] * 6).fill(L.TABLE_FILL | PP | ALL_FLAGS)
    off = pair_offset(6, PP | ALL_FLAGS)
    assert off == HDR + 6 * (ROW + L.TABLE_NOISE_BYTES + L.TABLE_BLEND_BYTES + L.TABLE_APG_BYTES)
    assert off + 6 * REC == L.table_bytes(6, PP | ALL_FLAGS) == L.table_bytes(6, PP | PR | ALL_FLAGS)
    c.check_run(0, range(6))
    assert c.poison(HDR + 6 * ROW, off) and c.poison(off + 6 * REC)


def test_pair_rows_and_perp_rows_of_one_call_land_in_different_runs_and_one_section():
    order, left, i = [], {"ode": 20, "pair": 12, "perp": 12, "zst": 5}, 0
    while any(left.values()):
        k = ("ode", "pair", "perp", "ode", "zst", "perp", "pair")[i % 7]
        i += 1
        if left[k]:
            left[k] -= 1
            order.append(k)
    c = PerpCall(order).fill(L.TABLE_FILL | PR | PP | ALL_FLAGS)
    R = len(order)
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 4]
    first = 0
    for k in sorted(set(order), key=order.index):
        members = [r for r, kk in enumerate(order) if kk == k]
        c.check_run(first, members)
        first += len(members)
    assert first == R
    off = pair_offset(R, PR | PP | ALL_FLAGS)                      # ONE section: 24 records beside the 24 rows of the two kinds
    recs = c.bytes()[off:off + R * REC].reshape(R, REC)
    assert sum(1 for i in range(R) if not bool((recs[i] == POISON).all())) == 24
    # a Perp-Neg request of another model type or prologue opens a run of its own (het_same_group's keys); so does another batch
    c = PerpCall(["perp"] * 6)
    c.st[2].model_type = L.MODEL["v"]
    c.st[4].flags &= ~L.F_TO_X0
    c.bs[5].batch = 2
    c.fill()
    assert c.header()[2:] == [6, 4]
    c.check_run(0, [0, 1, 3])
    c.check_run(3, [2])
    c.check_run(4, [4])
    c.check_run(5, [5])


def _ragged(c, r):
    """a sample of 12 elements: whole 8-element groups for a pair row (n = 24), none for a Perp-Neg row"""
    c.bs[r].n, c.bs[r].batch = 24, 2


@pytest.mark.parametrize("mode", [L.TABLE_FILL | PP, L.TABLE_FILL | PP | PR])
@pytest.mark.parametrize("what", ["ragged", "n % 8", "misaligned", "misaligned g", "separate xe", "ss3t"])
def test_a_flagged_request_without_copies_that_fails_the_predicate_goes_alone(what, mode):
    """no row, no error, the others' rows what they are without it -- and never a pair row, which would blend it linearly"""
    c = PerpCall(["perp"] * 9)
    c.bs[5].x_out2 = c.bs[5].thr_hint = None
    _ragged(c, 5) if what == "ragged" else _disqualify(c, 5, what)
    c.fill(mode)
    others = [r for r in range(9) if r != 5]
    assert c.header()[2:] == [9, 1]
    c.check_run(0, others)
    assert c.poison(HDR + 8 * ROW, pair_offset(9, mode)) and c.poison(pair_offset(9, mode) + 8 * REC)
    # (the same request without the flag is a pair row of a DPM_TABLE_PAIR call where n is whole groups)
    if what == "ragged" and mode & PR:
        c.st[5].flags &= ~PERP
        c.table[:] = POISON
        c.fill(mode)
        assert c.header()[2:] == [9, 2]


def test_the_copies_three_errors_and_their_order():
    for mode, both in ((PP, BOTH_PP), (PP | PR, BOTH)):
        # one copy without the other
        for which in ("x_out2", "thr_hint"):
            c = PerpCall(["perp"] * 9)
            assert c.bs[4].x_out2 and c.bs[4].thr_hint
            setattr(c.bs[4], which, None)
            before = c.table.copy()
            for m in (L.TABLE_FILL | mode, L.TABLE_LAUNCH | mode):
                rc, msg = c.run(m)
                assert (rc, msg) == (L.ERR_ARG, both), (which, m, rc, msg)
                assert np.array_equal(c.table, before)
        # copies on a request that owns neither a pair row nor a Perp-Neg row: the lone kernel's refusal, for the whole call
        for what in ("ragged", "n % 8", "misaligned", "misaligned g", "separate xe", "ss3t"):
            c = PerpCall(["perp"] * 9)
            assert c.bs[4].x_out2
            _ragged(c, 4) if what == "ragged" else _disqualify(c, 4, what)
            before = c.table.copy()
            rc, msg = c.run(L.TABLE_FILL | mode)
            assert (rc, msg) == (L.ERR_UNSUPPORTED, X_OUT2), (what, rc, msg)
            assert np.array_equal(c.table, before)
        for which in ("x_out2", "thr_hint"):                       # a misaligned copy is no row either
            c = PerpCall(["perp"] * 9)
            setattr(c.bs[4], which, getattr(c.bs[4], which) + 8)
            before = c.table.copy()
            rc, msg = c.run(L.TABLE_FILL | mode)
            assert (rc, msg) == (L.ERR_UNSUPPORTED, X_OUT2) and np.array_equal(c.table, before)
        # every request is checked before anything is written: the LAST one's missing copy refuses the call
        c = PerpCall(["perp"] * 9)
        c.bs[8].thr_hint = None
        before = c.table.copy()
        rc, msg = c.run(L.TABLE_FILL | mode)
        assert (rc, msg) == (L.ERR_ARG, both) and np.array_equal(c.table, before)
    # the order of a record's own checks: remedy flags, then the guidance's, then the flag's, then the copies'
    c = PerpCall(["perp"] * 9)
    c.st[3].flags |= L.F_CFG_ZSTAR
    rc, msg = c.run(L.TABLE_FILL | PP)
    assert rc == L.ERR_ARG and "DPM_F_CFG_ZSTAR is valid under classifier-free guidance only" in msg
    c = PerpCall(["perp"] * 9)
    c.st[3].cg_scale = float("inf")
    c.bs[3].thr_hint = None
    rc, msg = c.run(L.TABLE_FILL | PP)
    assert rc == L.ERR_ARG and "both must be finite" in msg
    c = PerpCall(["perp"] * 9)
    c.bs[3].g = None
    rc, msg = c.run(L.TABLE_FILL | PP)
    assert rc == L.ERR_ARG and "DPM_GUIDE_CFG2 needs e1 and g" in msg
    # an unflagged two-condition request of a call with DPM_TABLE_PERP alone may carry no copy: version 218's text
    c = PerpCall(["perp"] * 8 + ["pair"])
    assert c.bs[8].x_out2
    before = c.table.copy()
    rc, msg = c.run(L.TABLE_FILL | PP)
    assert (rc, msg) == (L.ERR_UNSUPPORTED, X_OUT2) and np.array_equal(c.table, before)


def test_without_the_flag_every_call_is_version_220s():
    # a flagged request in a table-mode call without DPM_TABLE_PERP: the old refusal, nothing written
    for mode in (L.TABLE_FILL, L.TABLE_FILL | PR, L.TABLE_LAUNCH | PR | ALL_FLAGS):
        c = PerpCall(["pair"] * 4 + ["perp"] + ["pair"] * 4)
        c.bs[4].x_out2 = c.bs[4].thr_hint = None
        if not mode & PR:
            for r in range(9):
                c.bs[r].x_out2 = c.bs[r].thr_hint = None
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert (rc, msg) == (L.ERR_UNSUPPORTED, NO_ROWS), (mode, rc, msg)
        assert np.array_equal(c.table, before)
    # plain and two-condition requests: with and without the new bit the table is byte for byte the same
    kinds = [("ode", "pair")[r % 2] for r in range(40)]
    for mode in (L.TABLE_FILL | PR, L.TABLE_FILL | PR | L.TABLE_NOISE, L.TABLE_FILL | PR | ALL_FLAGS):
        c = PerpCall(kinds).fill(mode)
        was = c.bytes()[:c.size].copy()
        assert c.header()[2:] == [40, 2]
        c.table[:] = POISON
        c.fill(mode | PP)
        assert np.array_equal(c.bytes()[:c.size], was)
        assert L.table_bytes(40, mode) == L.table_bytes(40, mode | PP)
