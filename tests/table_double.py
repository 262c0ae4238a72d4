"""CPU double of the slab pool's device side -- TEST INFRASTRUCTURE, installed on top of unipc_double.install_unipc_double.

dpm_stage_launch_multi in table mode: DPM_TABLE_FILL goes to the REAL library (it makes no HIP call and writes host memory
only), DPM_TABLE_LAUNCH checks the table it is handed -- a byte copy of what FILL wrote -- and runs the per-request numpy
doubles; mode 0 runs the doubles alone.  The pinning and copy hooks of dpm_solver_amd/_device.py become plain CPU tensors and
a synchronous copy (a CPU-only machine cannot pin)."""
import ctypes as C

import numpy as np
import torch

import kernel_double as KD
import unipc_double as UD
from dpm_solver_amd import _lib as L

CALLS = []          # (requests, table_mode) of every multi-request call
COPIES = []         # bytes of every host-to-device copy
FILLED = {}         # host table pointer -> its bytes after FILL (what the copy must carry)


def launch_raw(st_ref, b_ref, stream):
    if st_ref._obj.form == L.FORM_UNIPC:
        return UD.launch_raw_double(st_ref, b_ref, stream)
    return KD.launch_raw_double(st_ref, b_ref, stream)


def _table_bytes(ptr, n_req):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (L.TABLE_HEADER_BYTES + n_req * L.TABLE_ROW_BYTES,))


def launch_multi_table(st, bufs, n_req, stream):
    o = bufs[0].opts.contents
    assert o.per_request_stages == 1
    n_req, mode = int(n_req), int(o.table_mode)
    CALLS.append((n_req, mode))
    if mode == L.TABLE_FILL:
        rc = L.lib.dpm_stage_launch_multi(st, bufs, n_req, None)
        FILLED["last"] = _table_bytes(bufs[0].workspace, n_req).copy()
        return rc
    if mode == L.TABLE_LAUNCH:
        tab = _table_bytes(bufs[0].workspace, n_req)
        assert np.array_equal(tab[:16], FILLED["last"][:16]) and tab[:16].view(np.uint32)[0] == L.TABLE_MAGIC, "stale table"
        assert np.array_equal(tab, FILLED["last"]), "the device table is not a byte copy of what DPM_TABLE_FILL wrote"
    for r in range(n_req):
        rc = launch_raw(KD._Ref(st[r]), KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


def _copy(dst, src):
    COPIES.append(int(src.numel()))
    dst.copy_(src)
    return None


def install_table_double(monkeypatch, S, D):
    UD.install_unipc_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    monkeypatch.setattr(S, "_pinned_bytes", lambda n: torch.zeros(int(n), dtype=torch.uint8))
    monkeypatch.setattr(S, "_device_bytes", lambda n, dev: torch.zeros(int(n), dtype=torch.uint8))
    monkeypatch.setattr(S, "_copy_to_device", _copy)
    monkeypatch.setattr(S, "_event_wait", lambda ev: None)
    CALLS.clear()
    COPIES.clear()
    FILLED.clear()
