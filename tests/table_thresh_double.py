"""CPU double of a thresholding slab pool's device side -- TEST INFRASTRUCTURE, table_double.py with DPM_TABLE_THRESH on the mode.

DPM_TABLE_FILL | DPM_TABLE_THRESH goes to the REAL library (host memory, no HIP call), the LAUNCH call checks that its table is
a byte copy of what FILL wrote, that every row of the call is in it -- the table's header says how many runs it holds, the rows
are read back and matched against the requests' pointers -- and runs the per-request numpy doubles (kernel_double handles
DPM_F_THRESH).  Modes 1 / 2 and 0 go as in table_double."""
import numpy as np

import kernel_double as KD
import table_double as TD
from dpm_solver_amd import _lib as L

CALLS, COPIES, FILLED = TD.CALLS, TD.COPIES, TD.FILLED
ROWS = []           # per LAUNCH call: (runs in the header, the x pointers of its rows in table order)
FLAGS = L.TABLE_NOISE | L.TABLE_THRESH


def launch_multi_table(st, bufs, n_req, stream):
    o = bufs[0].opts.contents
    assert o.per_request_stages == 1
    n_req, mode = int(n_req), int(o.table_mode)
    CALLS.append((n_req, mode))
    if mode & ~FLAGS == L.TABLE_FILL:
        rc = L.lib.dpm_stage_launch_multi(st, bufs, n_req, None)
        FILLED["last"] = TD._table_bytes(bufs[0].workspace, n_req).copy()
        return rc
    if mode & ~FLAGS == L.TABLE_LAUNCH:
        tab = TD._table_bytes(bufs[0].workspace, n_req)
        assert tab[:16].view(np.uint32)[0] == L.TABLE_MAGIC, "stale table"
        assert np.array_equal(tab, FILLED["last"]), "the device table is not a byte copy of what DPM_TABLE_FILL wrote"
        body = tab[L.TABLE_HEADER_BYTES:].reshape(n_req, L.TABLE_ROW_BYTES)
        ROWS.append((int(tab[:16].view(np.uint32)[3]), body[:, :8].copy().view(np.uint64).ravel().tolist()))
    for r in range(n_req):
        rc = TD.launch_raw(KD._Ref(st[r]), KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


def install_table_thresh_double(monkeypatch, S, D):
    TD.install_table_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    ROWS.clear()
