"""CPU double of an adaptive-projected-guidance slab pool's device side -- TEST INFRASTRUCTURE, table_double.py with
DPM_TABLE_APG on the mode.

DPM_TABLE_FILL | DPM_TABLE_APG goes to the REAL library (host memory, no HIP call); the LAUNCH call checks that its table is a
byte copy of what FILL wrote, records the runs its header counts and the rows it holds -- their x pointers and flags -- and
checks every row's APG record at the documented offset, word for word: the running average (the request's thr_hint; null
without a momentum), eta, r, beta, three zero words; the record slot of a row that is no run's stays poisoned.  Then the
per-request numpy doubles run: apg_double's for a request with DPM_F_CFG_APG -- on a copy of its buffers whose workspace is its
thr_hint, as the library launches a request of such a call, its inputs checked decidable first --, table_double's for every
other one.  The single-request entry points (sample() of the comparison solvers) get the same doubles."""
import ctypes as C

import numpy as np

import apg_double as AD
import kernel_double as KD
import table_double as TD
from dpm_solver_amd import _lib as L

CALLS, COPIES, FILLED = TD.CALLS, TD.COPIES, TD.FILLED
# per LAUNCH call: (runs in the header, [(x pointer, flags, average pointer, (eta, r, beta))] of its rows in table order,
# [(flags, cfg_scale, cg_scale, thr_ratio, thr_max, thr_hint)] of every request of the call)
ROWS = []
POISON = 0xAB
FLAGS = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_RESCALE | L.TABLE_APG


def table_view(ptr, n_req, flags):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (L.table_bytes(n_req, flags),))


def apg_offset(n_req, flags):
    """where the APG section of a call of n_req requests starts (include/dpm_hip.h, "Table mode")"""
    return (L.TABLE_HEADER_BYTES + n_req * L.TABLE_ROW_BYTES + (n_req * L.TABLE_NOISE_BYTES if flags & L.TABLE_NOISE else 0)
            + (n_req * L.TABLE_BLEND_BYTES if flags & L.TABLE_BLEND else 0))


def record(tab, n_req, flags, i):
    """(average pointer, eta, r, beta bits, the three trailing words) of the APG record beside table row i"""
    raw = tab[apg_offset(n_req, flags) + i * L.TABLE_APG_BYTES:][:L.TABLE_APG_BYTES].copy()
    w = raw.view(np.uint32)
    return int(raw[:8].view(np.uint64)[0]), tuple(int(v) for v in w[2:5]), tuple(int(v) for v in w[5:8])


def bits(v):
    return int(np.float32(v).view(np.uint32))


def with_hint_as_workspace(b):
    bb = L.Buffers.from_buffer_copy(b)
    bb.workspace = b.thr_hint
    return bb


def launch_raw(st_ref, b_ref, stream):
    if st_ref._obj.flags & L.F_CFG_APG:
        return AD.launch_raw_double(st_ref, b_ref, stream)
    return TD.launch_raw(st_ref, b_ref, stream)


def launch_stage(st, *a, **kw):
    if st.flags & L.F_CFG_APG:
        return AD.launch_stage_double(st, *a, **kw)
    return TD.UD.launch_stage_double(st, *a, **kw)


def launch_multi_table(st, bufs, n_req, stream):
    o = bufs[0].opts.contents
    assert o.per_request_stages == 1
    n_req, mode = int(n_req), int(o.table_mode)
    CALLS.append((n_req, mode))
    flags = mode & FLAGS
    if mode & ~FLAGS == L.TABLE_FILL:
        table_view(bufs[0].workspace, n_req, flags)[L.TABLE_HEADER_BYTES:] = POISON      # (a slot FILL leaves alone is no row)
        rc = L.lib.dpm_stage_launch_multi(st, bufs, n_req, None)
        FILLED["last"] = table_view(bufs[0].workspace, n_req, flags).copy()
        return rc
    if mode & ~FLAGS == L.TABLE_LAUNCH:
        tab = table_view(bufs[0].workspace, n_req, flags)
        assert tab[:16].view(np.uint32)[0] == L.TABLE_MAGIC, "stale table"
        assert np.array_equal(tab, FILLED["last"]), "the device table is not a byte copy of what DPM_TABLE_FILL wrote"
        body = tab[L.TABLE_HEADER_BYTES:L.TABLE_HEADER_BYTES + n_req * L.TABLE_ROW_BYTES].reshape(n_req, L.TABLE_ROW_BYTES)
        ptr = body[:, :8].copy().view(np.uint64).ravel()
        by_x = {int(bufs[r].x): r for r in range(n_req)}
        rows = []
        for i in range(n_req):
            rec_raw = tab[apg_offset(n_req, flags) + i * L.TABLE_APG_BYTES:][:L.TABLE_APG_BYTES]
            if bool((body[i] == POISON).all()):
                assert bool((rec_raw == POISON).all()), "a record beside a slot that is no row"
                continue
            r = by_x[int(ptr[i])]
            if not (flags & L.TABLE_APG) or not st[r].flags & L.F_CFG_APG:
                assert not (flags & L.TABLE_APG) or bool((rec_raw == POISON).all()), "a record beside a row that is no APG row"
                rows.append((int(ptr[i]), int(st[r].flags), 0, None))
                continue
            avg, par, zeros = record(tab, n_req, flags, i)
            want = int(bufs[r].thr_hint or 0) if st[r].thr_max != 0 else 0
            assert (avg, par, zeros) == (want, (bits(st[r].cg_scale), bits(st[r].thr_ratio), bits(st[r].thr_max)), (0, 0, 0)), \
                (i, r, hex(avg), par, zeros)
            rows.append((int(ptr[i]), int(st[r].flags), avg, (float(st[r].cg_scale), float(st[r].thr_ratio), float(st[r].thr_max))))
        ROWS.append((int(tab[:16].view(np.uint32)[3]), rows,
                     [(int(st[r].flags), float(st[r].cfg_scale), float(st[r].cg_scale), float(st[r].thr_ratio),
                       float(st[r].thr_max), int(bufs[r].thr_hint or 0)) for r in range(n_req)]))
    for r in range(n_req):
        b = bufs[r]
        if (flags & L.TABLE_APG) and (st[r].flags & L.F_CFG_APG) and st[r].thr_max != 0:
            assert b.thr_hint, "a momentum in a DPM_TABLE_APG call needs the running average in thr_hint"
            b = with_hint_as_workspace(b)            # (as the library launches a request of such a call on its own)
        rc = launch_raw(KD._Ref(st[r]), KD._Ref(b), stream)
        if rc:
            return rc
    return 0


def install_table_apg_double(monkeypatch, S, D):
    TD.install_table_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_launch_stage", launch_stage)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    ROWS.clear()
