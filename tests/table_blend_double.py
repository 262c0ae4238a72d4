"""CPU double of an inpainting slab pool's device side -- TEST INFRASTRUCTURE, table_double.py and kernel_double.blend composed.

dpm_stage_launch_multi with DPM_TABLE_BLEND on the mode: DPM_TABLE_FILL | DPM_TABLE_BLEND goes to the REAL library (host memory,
no HIP call), the LAUNCH call checks that its table -- rows AND blend records -- is a byte copy of what FILL wrote and runs the
per-request doubles, a DPM_F_BLEND request through kernel_double's KExt epilogue (launch_raw_double(allow_blend=True)).
dpm_blend_launch -- the blend of x_T on the tick that admits a request -- is kernel_double.blend on the raw addresses.
Modes 1 / 2 and 0 go as in table_double.  With DPM_TABLE_NOISE on the mode as well (a pool built with sde=True, inpaint=True) the
table carries the noise section in front of the blend section and an SDE row goes through table_sde_double.launch_row."""
import ctypes as C

import numpy as np

import kernel_double as KD
import table_double as TD
import table_sde_double as TSD
import unipc_double as UD
from dpm_solver_amd import _lib as L

CALLS, COPIES, FILLED = TD.CALLS, TD.COPIES, TD.FILLED
RUNS = []           # per LAUNCH call: (runs in the table's header, rows with DPM_F_BLEND, rows without)
BLENDS = []         # (elements, period) of every stand-alone blend launch


def launch_raw(st_ref, b_ref, stream):
    if st_ref._obj.form == L.FORM_UNIPC:
        return UD.launch_raw_double(st_ref, b_ref, stream)
    return KD.launch_raw_double(st_ref, b_ref, stream, allow_blend=True)


def _table_bytes(ptr, n_req, blend, noise=False):
    size = L.TABLE_HEADER_BYTES + n_req * (L.TABLE_ROW_BYTES + (L.TABLE_NOISE_BYTES if noise else 0)
                                           + (L.TABLE_BLEND_BYTES if blend else 0))
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (size,))


def launch_multi_table(st, bufs, n_req, stream):
    o = bufs[0].opts.contents
    assert o.per_request_stages == 1
    n_req, mode = int(n_req), int(o.table_mode)
    CALLS.append((n_req, mode))
    blend, noise = bool(mode & L.TABLE_BLEND), bool(mode & L.TABLE_NOISE)
    base = mode & ~(L.TABLE_BLEND | L.TABLE_NOISE)
    if base == L.TABLE_FILL:
        rc = L.lib.dpm_stage_launch_multi(st, bufs, n_req, None)
        FILLED["last"] = _table_bytes(bufs[0].workspace, n_req, blend, noise).copy()
        return rc
    if base == L.TABLE_LAUNCH:
        tab = _table_bytes(bufs[0].workspace, n_req, blend, noise)
        assert tab[:16].view(np.uint32)[0] == L.TABLE_MAGIC, "stale table"
        assert np.array_equal(tab, FILLED["last"]), "the device table is not a byte copy of what DPM_TABLE_FILL wrote"
        nb = sum(1 for r in range(n_req) if st[r].flags & L.F_BLEND)
        RUNS.append((int(tab[:16].view(np.uint32)[3]), nb, n_req - nb))
    for r in range(n_req):
        assert blend or not (st[r].flags & L.F_BLEND)
        if st[r].flags & L.F_NOISE:
            assert noise and not (st[r].flags & L.F_BLEND)
            rc = TSD.launch_row(KD._Ref(st[r]), KD._Ref(bufs[r]), stream)
        else:
            assert not bufs[r].noise_sample0
            rc = launch_raw(KD._Ref(st[r]), KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


def blend_launch(x, mask, a, b, alpha, sigma, out, n, period, dtype, stream):
    """dpm_blend_launch on raw addresses: out = x*mask + (1 - mask)*(alpha*a + sigma*b), mask indexed i % period"""
    n, period = int(n), int(period)
    assert n % period == 0 and out != x, "the stand-alone blend is not run in place"
    BLENDS.append((n, period))
    m = np.tile(KD._rd(mask, period, dtype), n // period)
    res = KD.blend(alpha, sigma, KD._rd(x, n, dtype), m, KD._rd(a, n, dtype), KD._rd(b, n, dtype) if b else None)
    KD._wr(out, res, dtype)
    return 0


def install_table_blend_double(monkeypatch, S, D):
    TD.install_table_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    monkeypatch.setattr(S, "_blend_launch_raw", blend_launch)
    RUNS.clear()
    BLENDS.clear()


def install_table_blend_sde_double(monkeypatch, S, D):
    """a pool built with sde=True AND inpaint=True: table_sde_double's doubles, the table walk and the blend of this module"""
    TSD.install_table_sde_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    monkeypatch.setattr(S, "_blend_launch_raw", blend_launch)
    RUNS.clear()
    BLENDS.clear()
