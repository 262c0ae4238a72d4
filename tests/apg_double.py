"""numpy test double of an adaptive-projected-guidance stage (DPM_F_CFG_APG, include/dpm_hip.h) -- TEST INFRASTRUCTURE, never
imported by the product.  A restatement of the contract on top of kernel_double's `to_noise` / `combine`:

    c, u = x0 of the conditional / unconditional raw output on xe      fp32: to_noise, then (xe - sigma_e * eps) / alpha_e
    d    = c - u;   beta != 0:  a = d + beta * a, a stored, d = a        fp32
    S_dd, S_dc, S_cc                                                    products and sums in double
    sc64 = r > 0 ? (t < 1 ? t : 1) : 1, t = r / sqrt(S_dd);  sc = fp32(sc64);  q = fp32((sc64 * S_dc) / S_cc)
    upd  = (sc * d - q * c) + eta * (q * c);   mn = c + (s - 1) * upd   fp32
    combine (fp32 model values); store

The kernel may add its doubles in any order.  `scalars` therefore computes (sc, q) THREE ways -- a sequential double sum,
numpy's pairwise sum and math.fsum (the exactly rounded sum) -- and `assert_inputs_decidable` fails a test ON THE CPU when the
three disagree in any bit of either for any sample: a precondition on the chosen inputs, under which a correct kernel cannot
differ from this double through summation order.  No sample is skipped.
"""
import numpy as np
import torch

import kernel_double as KD
from dpm_solver_amd import _lib as L
from rescale_double import SUMS

F32, F64 = np.float32, np.float64


def params(st):
    """(eta, r, beta) of a flagged stage record, fp32"""
    return F32(st.cg_scale), F32(st.thr_ratio), F32(st.thr_max)


def x0_of(o, xe, c):
    """the data prediction of one raw output (flat fp32 arrays): the model value of a flag-less data-prediction stage"""
    with np.errstate(all="ignore"):
        eps = KD.to_noise(o, xe, c)
        return ((xe - c.sigma_e * eps) / c.alpha_e).astype(F32)


def direction(st, xe, e0, e1, avg):
    """(c, d, new average or None) of a launch: flat fp32 arrays; avg: the running average going in (None: beta == 0)"""
    c = KD._Coef(st)
    beta = params(st)[2]
    cc = x0_of(e0, xe, c)
    d = (cc - x0_of(e1, xe, c)).astype(F32)
    if beta != 0:
        with np.errstate(all="ignore"):
            a = (d + (beta * avg).astype(F32)).astype(F32)
        return cc, a, a
    return cc, d, None


def scalars(c, d, r, how="seq"):
    """(sc, q) of every sample: c, d are [B, P] fp32 arrays, r the fp32 threshold; returns two arrays of B fp32 values"""
    sc, q = [], []
    with np.errstate(all="ignore"):
        for b in range(c.shape[0]):
            d64, c64 = d[b].astype(F64), c[b].astype(F64)
            s_dd, s_dc, s_cc = SUMS[how](d64 * d64), SUMS[how](d64 * c64), SUMS[how](c64 * c64)
            sc64 = F64(1.0)
            if r > 0:
                t = F64(r) / np.sqrt(s_dd)
                sc64 = t if t < 1.0 else F64(1.0)
            sc.append(F32(sc64))
            q.append(F32((sc64 * s_dc) / s_cc))
    return np.array(sc, dtype=F32), np.array(q, dtype=F32)


def assert_inputs_decidable(st, xe, e0, e1, avg, batch):
    """the precondition of a bit-exact comparison: sc and q do not depend on the summation order for these inputs (flat fp32
    arrays of `batch` samples; avg: the running average going in, or None)"""
    cc, d, _ = direction(st, xe, e0, e1, avg)
    r = params(st)[1]
    got = {how: scalars(cc.reshape(batch, -1), d.reshape(batch, -1), r, how) for how in SUMS}
    for how in ("np", "fsum"):
        for i, name in enumerate(("sc", "q")):
            same = got[how][i].view(np.uint32) == got["seq"][i].view(np.uint32)
            assert bool(same.all()), "%s depends on the summation order for sample %d: %s" % (
                name, int(np.nonzero(~same)[0][0]), {k: v[i].tolist() for k, v in got.items()})


def stage(st, x, xe, e0, e1, h1, h2, avg, batch):
    """(x_out, mn, new average or None) of one flagged stage on flat fp32 arrays"""
    c = KD._Coef(st)
    assert st.flags & L.F_CFG_APG and st.flags & L.F_TO_X0 and c.guidance == L.GUIDE["classifier-free"]
    eta, r, _ = params(st)
    n = e0.size
    cc, d, new_avg = direction(st, xe, e0, e1, avg)
    cb, db = cc.reshape(batch, -1), d.reshape(batch, -1)
    sc, q = scalars(cb, db, r)
    with np.errstate(all="ignore"):
        dn, par = (sc.reshape(batch, 1) * db).astype(F32), (q.reshape(batch, 1) * cb).astype(F32)
        upd = ((dn - par).astype(F32) + (eta * par).astype(F32)).astype(F32)
        mn = (cb + ((c.cfg_scale - F32(1.0)) * upd).astype(F32)).astype(F32).reshape(n)
        out = KD.combine(c, x, mn, h1, h2, None)     # (model values are fp32: no half differences)
    return np.broadcast_to(out, (n,)).astype(F32), mn, new_avg


def _rd_avg(ptr, n):
    return KD._rd(ptr, n, L.DTYPE_F32) if ptr else None


def launch_raw_double(st_ref, b_ref, stream=None, check=True):
    """pointer-level double of dpm_stage_launch: a flagged stage here (the inputs checked decidable unless check=False),
    every other stage kernel_double's"""
    st, b = st_ref._obj, b_ref._obj
    if not (st.flags & L.F_CFG_APG):
        return KD.launch_raw_double(st_ref, b_ref, stream)
    n, B = int(b.n), int(b.batch)
    sd, ed = b.state_dtype, b.eps_dtype
    assert sd != L.DTYPE_F64 and (not b.eps_stride or b.eps_stride == n // B)
    x, xe = KD._rd(b.x, n, sd), KD._rd(b.xe, n, sd)
    xe = x if xe is None else xe
    x = xe if x is None else x
    e0, e1 = KD._rd(b.e0, n, ed), KD._rd(b.e1, n, ed)
    mom = params(st)[2] != 0
    assert not mom or b.workspace, "a momentum needs the running average in workspace"
    avg = _rd_avg(b.workspace, n) if mom else None
    if check:
        assert_inputs_decidable(st, xe, e0, e1, avg, B)
    out, mn, new_avg = stage(st, x, xe, e0, e1, KD._rd(b.h1, n, sd), KD._rd(b.h2, n, sd), avg, B)
    if mom:
        KD._wr(b.workspace, new_avg, L.DTYPE_F32)
    KD._wr(b.x_out, out, sd)
    if b.x_out2:
        KD._wr(b.x_out2, out, sd)
    if st.flags & L.F_STORE_M:
        KD._wr(b.m_out, mn, sd)
    return 0


def launch_multi_double(st_ref, bufs, n_req, stream):
    """dpm_stage_launch_multi: one stage for every request, or -- bufs[0].opts.per_request_stages -- one per request"""
    per = bool(bufs[0].opts) and bufs[0].opts.contents.per_request_stages == 1
    for r in range(int(n_req)):
        rc = launch_raw_double(KD._Ref(st_ref[r]) if per else st_ref, KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


def launch_stage_double(st, x, xe, e0, e1, g, h1, h2, state_dtype, want_m=None, ext=None, opts=None, coef64=None):
    """double of _device._launch_stage (the general loop): flagged stages here, everything else kernel_double's.  The running
    average is ext['apg_avg'], updated in place; without one a momentum starts from zero (a first step)."""
    if not (st.flags & L.F_CFG_APG):
        return KD.launch_stage_double(st, x, xe, e0, e1, g, h1, h2, state_dtype, want_m, ext, opts, coef64)
    assert state_dtype != torch.float64 and not (ext is not None and ext.get("blend") is not None)
    ref_t = x if x is not None else xe
    ed = e0.dtype
    if ed not in (torch.float32, torch.float16, torch.bfloat16) or (state_dtype != torch.float32 and ed != state_dtype):
        ed = state_dtype
    to = lambda t, dt: None if t is None else (t if t.dtype == dt else t.to(dt))
    flat = lambda t, dt: None if t is None else KD._np(to(t, dt)).reshape(-1)
    xn, xen = flat(x, state_dtype), flat(xe, state_dtype)
    xen = xn if xen is None else xen
    xn = xen if xn is None else xn
    B = int(ref_t.shape[0])
    e0n, e1n = flat(e0, ed), flat(e1, ed)
    mom = params(st)[2] != 0
    avg_t = ext.get("apg_avg") if ext is not None else None
    avg = None if not mom else (np.zeros(e0n.size, dtype=F32) if avg_t is None else avg_t.numpy().reshape(-1).copy())
    assert_inputs_decidable(st, xen, e0n, e1n, avg, B)
    out, mn, new_avg = stage(st, xn, xen, e0n, e1n, flat(h1, state_dtype), flat(h2, state_dtype), avg, B)
    if mom and avg_t is not None:
        avg_t.copy_(torch.from_numpy(new_avg).reshape(avg_t.shape))
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(state_dtype).reshape(ref_t.shape)
    x_out = conv(out)
    if ext is not None and ext.get("dup"):
        ext["x2"] = torch.cat([x_out, x_out])
        x_out = ext["x2"][:x_out.shape[0]]
    store = bool(st.flags & L.F_STORE_M) if want_m is None else want_m
    return x_out, (conv(mn) if store else None)


def install_apg_double(monkeypatch, S, D):
    """kernel_double.install_cpu_double + the projected-guidance stage behind every launch entry point"""
    KD.install_cpu_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_launch_stage", launch_stage_double)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw_double)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_double)
