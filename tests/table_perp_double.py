"""CPU double of a Perp-Neg slab pool's device side -- TEST INFRASTRUCTURE, table_pair_double.py with DPM_TABLE_PERP on the mode,
on top of perp_double.py as table_pair_double.py stands on its kind's double.

DPM_TABLE_FILL | DPM_TABLE_PERP goes to the REAL library (host memory, no HIP call); the LAUNCH call checks that its table --
header, rows and the pair section -- is a byte copy of what FILL wrote, records the runs its header counts and the rows it holds
(their x pointers, the two scale words, the flags word and the pair record beside each), and runs the per-request numpy doubles:
perp_double.stage for a flagged DPM_GUIDE_CFG2 request, then the two copies (x_out2 and, in such a call, thr_hint) as the table
kernel stores them; table_pair_double's for every other request.  The single-request entry points (sample() of the comparison
solvers) get perp_double's."""
import ctypes as C

import numpy as np

import kernel_double as KD
import perp_double as PP
import table_double as TD
import table_pair_double as TPD
from dpm_solver_amd import _lib as L

CALLS, COPIES, FILLED = TD.CALLS, TD.COPIES, TD.FILLED
# per LAUNCH call: (runs in the header, [(x pointer, cfg_scale, cg_scale, g, third copy)] of its Perp-Neg rows in table order)
ROWS = []
POISON = 0xAB
FLAGS = TPD.FLAGS | L.TABLE_PERP
PAIR = PP.PAIR
W_CFG, W_CG = TPD.W_CFG, TPD.W_CG


def pair_offset(n_req, flags):
    """the documented offset of the pair section (include/dpm_hip.h, "Table mode"): unchanged by DPM_TABLE_PERP"""
    return L.table_bytes(n_req, flags & ~(L.TABLE_PAIR | L.TABLE_PERP))


def _table_bytes(ptr, n_req, flags):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (L.table_bytes(n_req, flags),))


def row_stage(st, b, check=True):
    """the numpy double of one Perp-Neg row: perp_double's stage on the request without its copies, then the copies"""
    assert bool(b.x_out2) == bool(b.thr_hint), "one copy without the other"
    bare = L.Buffers.from_buffer_copy(bytes(b))
    bare.x_out2, bare.thr_hint = None, None
    rc = PP.launch_raw_double(KD._Ref(st), KD._Ref(bare), None, check)
    if rc == 0 and b.x_out2:
        out = KD._rd(b.x_out, int(b.n), b.state_dtype)
        KD._wr(b.x_out2, out, b.state_dtype)
        KD._wr(b.thr_hint, out, b.state_dtype)
    return rc


def launch_raw(st_ref, b_ref, stream, flags):
    """one request: a flagged stage through perp_double (its copies written as stage_perp_kernel_table writes them where the
    call carries DPM_TABLE_PERP), every other through table_pair_double"""
    st, b = st_ref._obj, b_ref._obj
    if not PP.flagged(st):
        return TPD.launch_raw(st_ref, b_ref, stream, bool(flags & L.TABLE_PAIR))
    if not flags & L.TABLE_PERP:
        return PP.launch_raw_double(st_ref, b_ref, stream)
    return row_stage(st, b)


def launch_multi_table(st, bufs, n_req, stream):
    o = bufs[0].opts.contents
    assert o.per_request_stages == 1
    n_req, mode = int(n_req), int(o.table_mode)
    CALLS.append((n_req, mode))
    flags = mode & FLAGS
    if mode & ~FLAGS == L.TABLE_FILL:
        _table_bytes(bufs[0].workspace, n_req, flags)[L.TABLE_HEADER_BYTES:] = POISON      # (a slot FILL leaves alone is no row)
        rc = L.lib.dpm_stage_launch_multi(st, bufs, n_req, None)
        FILLED["last"] = _table_bytes(bufs[0].workspace, n_req, flags).copy()
        return rc
    if mode & ~FLAGS == L.TABLE_LAUNCH:
        tab = _table_bytes(bufs[0].workspace, n_req, flags)
        assert tab[:16].view(np.uint32)[0] == L.TABLE_MAGIC, "stale table"
        assert np.array_equal(tab, FILLED["last"]), "the device table is not a byte copy of what DPM_TABLE_FILL wrote"
        body = tab[L.TABLE_HEADER_BYTES:L.TABLE_HEADER_BYTES + n_req * L.TABLE_ROW_BYTES].reshape(n_req, L.TABLE_ROW_BYTES)
        ptr, words = body[:, :64].copy().view(np.uint64), body[:, 64:].copy().view(np.uint32)
        off = pair_offset(n_req, flags)
        recs = tab[off:off + n_req * L.TABLE_PAIR_BYTES].reshape(n_req, L.TABLE_PAIR_BYTES)
        by_x = {int(bufs[r].x): r for r in range(n_req)}
        rows = []
        for i in range(n_req):
            if bool((body[i] == POISON).all()):
                continue
            r = by_x[int(ptr[i, 0])]
            if st[r].guidance != PAIR or not PP.flagged(st[r]) or not flags & L.TABLE_PERP:
                continue
            s, w = (float(words[i, k].view(np.float32)) for k in (W_CFG, W_CG))
            assert (s, w) == (float(st[r].cfg_scale), float(st[r].cg_scale)), (i, r, s, w)
            g, xo3 = (int(v) for v in recs[i].copy().view(np.uint64))
            assert (g, xo3) == (int(bufs[r].g or 0), int(bufs[r].thr_hint or 0)), (i, r)
            assert int(ptr[i, 7]) == int(bufs[r].x_out2 or 0)
            rows.append((int(ptr[i, 0]), s, w, g, xo3))
        ROWS.append((int(tab[:16].view(np.uint32)[3]), rows))
    for r in range(n_req):
        rc = launch_raw(KD._Ref(st[r]), KD._Ref(bufs[r]), stream, flags)
        if rc:
            return rc
    return 0


def install_table_perp_double(monkeypatch, S, D):
    TD.install_table_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_launch_stage", PP.launch_stage_double)
    monkeypatch.setattr(S, "_stage_launch_raw", PP.launch_raw_double)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    ROWS.clear()
