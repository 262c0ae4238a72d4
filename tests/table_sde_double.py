"""CPU double of an SDE slab pool's device side -- TEST INFRASTRUCTURE, table_double.py and sde_double.py composed.

dpm_stage_launch_multi with DPM_TABLE_NOISE on the mode: DPM_TABLE_FILL | DPM_TABLE_NOISE goes to the REAL library (host memory,
no HIP call), the LAUNCH call checks that its table -- rows AND noise records -- is a byte copy of what FILL wrote and runs the
per-request doubles, an SDE row with dpm_buffers.noise_sample0 = k on the z of elements k * per_sample onwards (the noise
contract indexes the request's whole tensor).  Modes 1 / 2 and 0 go as in table_double."""
import ctypes as C

import numpy as np

import kernel_double as KD
import sde_double as SD
import table_double as TD
import unipc_double as UD
from dpm_solver_amd import _lib as L

CALLS, COPIES, FILLED = TD.CALLS, TD.COPIES, TD.FILLED
BASES = []          # noise_sample0 of every SDE row advanced by a table call


def launch_raw(st_ref, b_ref, stream):
    """one request: UniPC, SDE (from block 0: what a launch of the request alone computes) or ODE"""
    st = st_ref._obj
    if st.form == L.FORM_UNIPC:
        return UD.launch_raw_double(st_ref, b_ref, stream)
    return SD.launch_raw_noise_double(st_ref, b_ref, stream)


def launch_row(st_ref, b_ref, stream):
    """one row of a table call: an SDE row starts its z at element noise_sample0 * per_sample"""
    st, b = st_ref._obj, b_ref._obj
    k = int(b.noise_sample0)
    if not (st.flags & L.F_NOISE):
        assert k == 0
        return launch_raw(st_ref, b_ref, stream)
    BASES.append(k)
    off = k * (int(b.n) // int(b.batch))
    src = SD.Z_SOURCE[0]
    SD.Z_SOURCE[0] = lambda seed, index, n: src(seed, index, off + n)[off:]
    try:
        return SD.launch_raw_noise_double(st_ref, b_ref, stream)
    finally:
        SD.Z_SOURCE[0] = src


def _table_bytes(ptr, n_req, noise):
    size = L.TABLE_HEADER_BYTES + n_req * (L.TABLE_ROW_BYTES + (L.TABLE_NOISE_BYTES if noise else 0))
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (size,))


def launch_multi_table(st, bufs, n_req, stream):
    o = bufs[0].opts.contents
    assert o.per_request_stages == 1
    n_req, mode = int(n_req), int(o.table_mode)
    CALLS.append((n_req, mode))
    noise = bool(mode & L.TABLE_NOISE)
    if mode & ~L.TABLE_NOISE == L.TABLE_FILL:
        rc = L.lib.dpm_stage_launch_multi(st, bufs, n_req, None)
        FILLED["last"] = _table_bytes(bufs[0].workspace, n_req, noise).copy()
        return rc
    if mode & ~L.TABLE_NOISE == L.TABLE_LAUNCH:
        tab = _table_bytes(bufs[0].workspace, n_req, noise)
        assert tab[:16].view(np.uint32)[0] == L.TABLE_MAGIC, "stale table"
        assert np.array_equal(tab, FILLED["last"]), "the device table is not a byte copy of what DPM_TABLE_FILL wrote"
    for r in range(n_req):
        assert noise or not bufs[r].noise_sample0
        rc = launch_row(KD._Ref(st[r]), KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


def install_table_sde_double(monkeypatch, S, D):
    TD.install_table_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    BASES.clear()
