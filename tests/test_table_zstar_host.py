"""The host half of CFG-Zero* rows in the table-driven launch (DPM_TABLE_ZSTAR, C ABI version 217): the real library's
DPM_TABLE_FILL through ctypes, no GPU, in the style of tests/test_table_apg_host.py.  With the flag every DPM_F_CFG_ZSTAR
request that passes zstar_row_ok owns a row -- a row like any other, no record --, from a group of one on, in runs of its own;
without the flag the call is version 216's.  Nothing here launches a kernel."""
import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_apg_host import Call, MODES_214, apg_offset
from test_table_host import HDR, N, POISON, ROW

ZST, APG, RSC = L.TABLE_ZSTAR, L.TABLE_APG, L.TABLE_RESCALE
MODES_215 = tuple(MODES_214) + tuple(m | APG for m in MODES_214)                # the 64 valid modes of version 215
ALL_FLAGS = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND | RSC | APG


class ZCall(Call):
    """test_table_apg_host.Call with a fourth kind, "zst": DPM_F_CFG_ZSTAR on a classifier-free record that is plain in every
    other field (the flag reads cfg_scale alone); forms rotate over LIN1 / TWO / MS3 / DENOISE, guidance scales over three
    values, STORE_M and x_out2 alternate, as for the other per-sample kinds"""

    def __init__(self, kinds, **kw):
        super().__init__(["rsc" if k == "zst" else k for k in kinds], **kw)
        for r, k in enumerate(kinds):
            if k == "zst":
                s = self.st[r]
                s.flags = (s.flags & ~L.F_CFG_RESCALE) | L.F_CFG_ZSTAR
                s.cg_scale = s.cfg_scale * s.sigma_e

    def fill(self, mode=L.TABLE_FILL | ZST):
        return super().fill(mode)


def test_abi_217_the_constants_and_the_modes():
    assert L.lib.dpm_version() >= 217
    assert ZST == 4096 and (L.TABLE_FILL, L.TABLE_LAUNCH, L.TABLE_NOISE, L.TABLE_THRESH, L.TABLE_BLEND, RSC, APG) == (1, 2, 4, 8, 32, 128, 512)
    assert [int(L.lib.dpm_sizeof(i)) for i in (7, 8, 9, 10, 11, 12, 13, 14, 15, 16)] == [16, 144, 0, 32, 0, 48, 0, 32, 0, 0]
    for flags in sorted({m & ~3 for m in MODES_215}):                        # every flag set: the kind has no section
        assert L.table_bytes(20, flags | ZST) == L.table_bytes(20, flags), flags
    assert L.table_bytes(20, ZST) == HDR + 20 * ROW
    valid = set(MODES_215) | {m | ZST for m in MODES_215}
    assert len(valid) == 128 and len(MODES_215) == 64
    for mode in list(range(4090, 4110 + 1024 + 1)) + [8192 | 1, 2048 | 4096 | 1, 1 << 30]:
        if mode in valid:
            continue
        c = ZCall(["zst"] * 20)
        before = c.table.copy()
        rc, msg = c.run(mode)
        assert rc == L.ERR_ARG and "table_mode=%d" % mode in msg, (mode, rc, msg)
        assert np.array_equal(c.table, before)
    assert sum(1 for m in range(4090, 4110 + 1024 + 1) if m in valid) == 64     # each of the 64 plus 4096 lies in the sweep
    for mode in (4096, 4096 | 3, 4096 | 16 | 1, 4096 | 64 | 2, 4096 | 256 | 1, 4096 | 1024 | 1, 4096 | 2048 | 2, 8192 | 4096 | 1):
        assert mode not in valid
    for base in MODES_215:                                         # every valid FILL mode with bit 4096 fills
        if not base & L.TABLE_FILL:
            continue
        c = ZCall(["zst"] * 20).fill(base | ZST)
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 20, 1], base
        c.check_run(0, range(20))
        assert c.poison(HDR + 20 * ROW), base                      # nothing but the rows: no record in any section


@pytest.mark.parametrize("R", [1, 2, 17])
@pytest.mark.parametrize("batch", [1, 3])
def test_a_group_of_one_owns_a_row(R, batch):
    c = ZCall(["zst"] * R, n=8, batch=batch, dt=L.DTYPE_F32).fill()
    assert c.header()[2:] == [R, 1]
    c.check_run(0, range(R))
    assert c.poison(HDR + R * ROW)
    c = ZCall(["ode"] * 10 + ["zst"]).fill()                       # ... beside a plain group too small for rows
    assert c.header()[2:] == [11, 1]
    c.check_run(0, [10])
    assert c.poison(HDR + ROW)


def test_the_row_carries_the_flag_and_the_guidance_scale():
    """table_fill_rows writes make_params of the record as it is: the flags word keeps DPM_F_CFG_ZSTAR, cfg_scale is the row's"""
    c = ZCall(["zst"] * 6).fill()
    _, words = c.rows(0, 6)
    for r in range(6):
        assert int(words[r, 1]) == c.st[r].flags and c.st[r].flags & L.F_CFG_ZSTAR
        assert int(words[r, 4]) == int(np.float32(c.st[r].cfg_scale).view(np.uint32))


def test_flagged_and_plain_requests_form_two_runs():
    kinds = [("ode", "zst", "zst", "ode", "zst")[r % 5] for r in range(100)]
    c = ZCall(kinds).fill()
    ode, z = [r for r in range(100) if kinds[r] == "ode"], [r for r in range(100) if kinds[r] == "zst"]
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 100, 2]
    c.check_run(0, ode)
    c.check_run(40, z)
    assert c.poison(HDR + 100 * ROW)
    assert {c.st[r].form for r in z} == {L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3, L.FORM_DENOISE}         # the four forms share a run
    assert len({c.st[r].cfg_scale for r in z}) == 3                                                   # ... so do the scales,
    assert {bool(c.st[r].flags & L.F_STORE_M) for r in z} == {True, False}                            # DPM_F_STORE_M
    assert {bool(c.bs[r].x_out2) for r in z} == {True, False}                                         # and the duplicate store


def test_zstar_groups_among_every_other_kind_with_all_six_flags():
    """four CFG-Zero* groups (noise, v, x_start, score networks) of 40, 17, 2 and 1 members interleaved with 20 plain, 5 rescale
    and 6 APG rows in a call that carries every flag: a run each in the order the groups open, members in call order, ONE row
    counter, the header counts the runs, and no record beside a CFG-Zero* row"""
    keys = {"a": ("noise", 40), "b": ("v", 17), "c": ("x_start", 2), "d": ("score", 1)}
    order = []
    left = {k: v[1] for k, v in keys.items()}
    left["ode"], left["rsc"], left["apg"] = 20, 5, 6
    i = 0
    while any(left.values()):
        k = ("ode", "a", "b", "a", "c", "rsc", "a", "d", "b", "apg")[i % 10]
        i += 1
        if left[k]:
            left[k] -= 1
            order.append(k)
    c = ZCall([k if k in ("ode", "rsc", "apg") else "zst" for k in order])
    for r, k in enumerate(order):
        if k in keys:
            c.st[r].model_type = L.MODEL[keys[k][0]]
    c.fill(L.TABLE_FILL | ZST | ALL_FLAGS)
    assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(order), 7]
    first = 0
    for k in sorted(set(order), key=order.index):                   # the runs in the order their groups open
        members = [r for r, kk in enumerate(order) if kk == k]
        c.check_run(first, members)                                 # (beside a row that is no APG row: an untouched record slot)
        first += len(members)
    R = len(order)
    assert first == R and c.poison(HDR + R * ROW, apg_offset(R, ALL_FLAGS))      # the noise and blend sections: untouched


def _disqualify(c, r, what):
    s, b = c.st[r], c.bs[r]
    if what == "per_sample 4":
        b.n, b.batch = 8, 2
    elif what == "per_sample 12":
        b.n, b.batch = 24, 2
    elif what == "misaligned":
        b.h1 = b.x + 8
        s.form = L.FORM_TWO
    elif what == "misaligned x_out2":
        b.x_out2 = b.x_out + (1 << 19) + 8
    elif what == "separate xe":
        b.xe = b.x + (1 << 19)
    elif what == "eps_stride":
        b.eps_stride = 2 * N
    elif what == "ss3t":
        s.form, b.h1, b.h2 = L.FORM_SS3T, b.x + (1 << 18), b.x + (1 << 17)
    elif what == "unipc":
        s.form, b.h1 = L.FORM_UNIPC, b.x + (1 << 18)
        s.flags |= L.F_UNIPC_P2
    elif what == "f64":
        b.state_dtype = b.eps_dtype = L.DTYPE_F64
    elif what == "thresholded":
        s.flags |= L.F_THRESH
    elif what == "rescale too":
        s.flags |= L.F_CFG_RESCALE
        s.cg_scale = 0.7


# what the call answers such a request: (code, text), None = it is accepted and goes as its own launch, which still projects
OUTSIDERS = {"per_sample 4": None, "per_sample 12": None, "misaligned": None, "misaligned x_out2": None, "separate xe": None,
             "ss3t": None,
             "eps_stride": (L.ERR_UNSUPPORTED, "DPM_F_CFG_ZSTAR with eps_stride=%d" % (2 * N)),   # (as dpm_stage_launch answers it)
             "unipc": (L.ERR_UNSUPPORTED, "DPM_FORM_UNIPC"),
             "f64": (L.ERR_UNSUPPORTED, "DPM_F_CFG_ZSTAR"),
             "thresholded": (L.ERR_UNSUPPORTED, "DPM_F_CFG_ZSTAR"),
             "rescale too": (L.ERR_UNSUPPORTED, "DPM_F_CFG_ZSTAR")}


@pytest.mark.parametrize("what", sorted(OUTSIDERS))
def test_a_flagged_request_that_fails_the_predicate_owns_no_row(what):
    c = ZCall(["zst"] * 21)
    _disqualify(c, 7, what)
    if OUTSIDERS[what] is not None:
        before = c.table.copy()
        rc, msg = c.run(L.TABLE_FILL | ZST)
        assert rc == OUTSIDERS[what][0] and OUTSIDERS[what][1] in msg, (rc, msg)      # the call reports it ...
        assert np.array_equal(c.table, before)                        # ... and writes nothing
        return
    c.fill()
    others = [r for r in range(21) if r != 7]
    assert c.header()[2:] == [21, 1]
    c.check_run(0, others)
    assert c.poison(HDR + 20 * ROW)
    ref = ZCall(["zst"] * 21).fill()                               # the others' rows: what they are without the outsider
    assert np.array_equal(c.rows(0, 20)[1], ref.rows(0, 21)[1][np.array(others)])


def test_a_row_of_other_n_batch_or_dtype_opens_its_own_run():
    c = ZCall(["zst"] * 12)
    c.bs[3].n, c.bs[3].batch = 2 * N, 2                            # another n and batch
    c.bs[4].n, c.bs[4].batch = 2 * N, 1                            # another n alone
    c.bs[5].state_dtype = L.DTYPE_F32                              # another pair: fp32 state, fp16 outputs
    c.st[8].model_type = L.MODEL["v"]
    c.st[9].flags &= ~L.F_TO_X0                                    # the noise-prediction form: DPM_F_TO_X0 is a grouping key
    c.fill()
    assert c.header()[2:] == [12, 6]
    c.check_run(0, [r for r in range(12) if r not in (3, 4, 5, 8, 9)])
    for i, r in enumerate((3, 4, 5, 8, 9)):
        c.check_run(7 + i, [r])
    assert c.poison(HDR + 12 * ROW)


def test_without_the_flag_every_call_is_version_216s():
    kinds = [("ode", "zst")[r % 2] for r in range(40)]
    for mode in (L.TABLE_FILL, L.TABLE_FILL | L.TABLE_NOISE, L.TABLE_FILL | ALL_FLAGS):
        c = ZCall(kinds).fill(mode)
        ode = list(range(0, 40, 2))
        assert c.header() == [L.TABLE_MAGIC, L.lib.dpm_version(), 40, 1]
        c.check_run(0, ode)
        assert c.poison(HDR + len(ode) * ROW), "a flagged request wrote a row without DPM_TABLE_ZSTAR"
        was = c.bytes()[HDR:HDR + len(ode) * ROW].copy()           # ... and the plain rows are byte for byte those the flag leaves
        c.table[:] = POISON
        c.fill(mode | ZST)
        assert c.header()[2:] == [40, 2] and np.array_equal(c.bytes()[HDR:HDR + len(ode) * ROW], was)
        c.check_run(20, list(range(1, 40, 2)))
    # a request's own error keeps mode 0's text, and nothing is written
    c = ZCall(["zst"] * 20)
    c.bs[11].e1 = None
    before = c.table.copy()
    rc, msg = c.run(L.TABLE_FILL | ZST)
    assert rc == L.ERR_ARG and "CFG needs e1" in msg and np.array_equal(c.table, before)
