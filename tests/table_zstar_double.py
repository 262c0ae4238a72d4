"""CPU double of a CFG-Zero* slab pool's device side -- TEST INFRASTRUCTURE, table_rescale_double.py with DPM_TABLE_ZSTAR on the
mode.

DPM_TABLE_FILL | DPM_TABLE_ZSTAR goes to the REAL library (host memory, no HIP call); the LAUNCH call checks that its table is
a byte copy of what FILL wrote, records the runs its header counts and the rows it holds -- their x pointers, flags and
cfg_scale words -- and runs the per-request numpy doubles: zstar_double.stage for a row with DPM_F_CFG_ZSTAR (its inputs checked
decidable first: a does not depend on the summation order), table_double's for every other row.  The single-request entry
points (sample() of the comparison solvers) get the same doubles."""
import numpy as np

import kernel_double as KD
import table_double as TD
import zstar_double as ZD
from dpm_solver_amd import _lib as L

CALLS, COPIES, FILLED = TD.CALLS, TD.COPIES, TD.FILLED
# per LAUNCH call: (runs in the header, [(x pointer, flags, cfg_scale)] of its rows in table order, [(flags, cfg_scale)] of every
# request of the call)
ROWS = []
POISON = 0xAB
FLAGS = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_RESCALE | L.TABLE_APG | L.TABLE_ZSTAR
# the words of a row's stage scalars the pool's per-request choice and guidance scale decide (read back from a row filled for a
# record with known values, see word_of)
_WORDS = {}


def word_of(name):
    """the index of `name` (flags / cfg_scale) among a row's 20 words of stage scalars, found by filling one row"""
    if not _WORDS:
        import ctypes as C
        st, b = L.Stage(), L.Buffers()
        st.form, st.flags, st.model_type, st.guidance = L.FORM_LIN1, L.F_TO_X0 | L.F_CFG_ZSTAR, L.MODEL["noise"], L.GUIDE["classifier-free"]
        st.alpha_e, st.sigma_e, st.cfg_scale, st.cg_scale = 0.75, 0.5, 7.25, 0.625
        arena = np.zeros(64, dtype=np.uint8)
        p = (arena.ctypes.data + 63) // 64 * 64
        b.x, b.e0, b.e1, b.x_out = p, p + (1 << 20), p + (2 << 20), p + (3 << 20)
        b.n, b.batch, b.state_dtype, b.eps_dtype = 64, 1, L.DTYPE_F32, L.DTYPE_F32
        o = L.LaunchOpts()
        o.per_request_stages, o.table_mode = 1, L.TABLE_FILL | L.TABLE_ZSTAR
        tab = np.zeros(L.table_bytes(1, L.TABLE_ZSTAR) + 16, dtype=np.uint8)
        off = (-tab.ctypes.data) % 16
        b.opts, b.workspace = C.pointer(o), tab.ctypes.data + off
        assert L.lib.dpm_stage_launch_multi(C.byref(st), C.byref(b), 1, None) == 0, L.lib.dpm_last_error()
        assert tab[off:off + 16].view(np.uint32)[3] == 1, "a lone CFG-Zero* request owns no row"
        words = tab[off + L.TABLE_HEADER_BYTES + 64:off + L.TABLE_HEADER_BYTES + L.TABLE_ROW_BYTES].view(np.uint32)
        for key, bits in (("flags", st.flags), ("cfg_scale", np.float32(7.25).view(np.uint32))):
            hit = np.flatnonzero(words == bits)
            assert len(hit) == 1, (key, words.tolist())
            _WORDS[key] = int(hit[0])
    return _WORDS[name]


def launch_raw(st_ref, b_ref, stream):
    if st_ref._obj.flags & L.F_CFG_ZSTAR:
        return ZD.launch_raw_double(st_ref, b_ref, stream)
    return TD.launch_raw(st_ref, b_ref, stream)


def launch_stage(st, *a, **kw):
    if st.flags & L.F_CFG_ZSTAR:
        return ZD.launch_stage_double(st, *a, **kw)
    return TD.UD.launch_stage_double(st, *a, **kw)


def launch_multi_table(st, bufs, n_req, stream):
    o = bufs[0].opts.contents
    assert o.per_request_stages == 1
    n_req, mode = int(n_req), int(o.table_mode)
    CALLS.append((n_req, mode))
    if mode & ~FLAGS == L.TABLE_FILL:
        TD._table_bytes(bufs[0].workspace, n_req)[L.TABLE_HEADER_BYTES:] = POISON      # (a slot FILL leaves alone is no row)
        rc = L.lib.dpm_stage_launch_multi(st, bufs, n_req, None)
        FILLED["last"] = TD._table_bytes(bufs[0].workspace, n_req).copy()
        return rc
    if mode & ~FLAGS == L.TABLE_LAUNCH:
        tab = TD._table_bytes(bufs[0].workspace, n_req)
        assert tab[:16].view(np.uint32)[0] == L.TABLE_MAGIC, "stale table"
        assert np.array_equal(tab, FILLED["last"]), "the device table is not a byte copy of what DPM_TABLE_FILL wrote"
        # the rows of the runs (a slot still poisoned belongs to no run): each is the row of one request of the call -- found
        # by its x pointer -- and carries that request's flags and cfg_scale
        body = tab[L.TABLE_HEADER_BYTES:].reshape(n_req, L.TABLE_ROW_BYTES)
        ptr, words = body[:, :8].copy().view(np.uint64).ravel(), body[:, 64:].copy().view(np.uint32)
        by_x = {int(bufs[r].x): r for r in range(n_req)}
        rows = []
        for i in range(n_req):
            if bool((body[i] == POISON).all()):
                continue
            r = by_x[int(ptr[i])]
            got = (int(words[i, word_of("flags")]), float(words[i, word_of("cfg_scale")].view(np.float32)))
            assert got == (int(st[r].flags), float(st[r].cfg_scale)), (i, r, got)
            rows.append((int(ptr[i]),) + got)
        ROWS.append((int(tab[:16].view(np.uint32)[3]), rows, [(int(st[r].flags), float(st[r].cfg_scale)) for r in range(n_req)]))
    for r in range(n_req):
        rc = launch_raw(KD._Ref(st[r]), KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


def install_table_zstar_double(monkeypatch, S, D):
    TD.install_table_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_launch_stage", launch_stage)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_table)
    ROWS.clear()
