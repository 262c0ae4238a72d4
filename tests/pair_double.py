"""numpy test double of a stage under guidance over two conditions (DPM_GUIDE_CFG2, include/dpm_hip.h) -- TEST INFRASTRUCTURE,
never imported by the product.  A restatement of the contract on top of kernel_double's `to_noise` / `combine`:

    n_k = to_noise(o_k, xe)                       k = 0 (condition), 1 (unconditional), 2 (second condition)
    d0 = n0 - n1;  d2 = n2 - n1
    eps = (n1 + s1 * d0) + s2 * d2                fp32, one rounding per operation; s1 = cfg_scale, s2 = cg_scale
    [eps -> x0]; combine (fp32 model values: nothing is rounded to the network's dtype after the loads); store

The arithmetic is elementwise: there is no summation order to decide, every input is comparable bit for bit.
"""
import numpy as np
import torch

import kernel_double as KD
from dpm_solver_amd import _lib as L

F32 = np.float32
PAIR = L.GUIDE["classifier-free-2"]


def blend(n0, n1, n2, s1, s2):
    """the five operations on fp32 arrays, each rounded once"""
    d0 = (n0 - n1).astype(F32)
    d2 = (n2 - n1).astype(F32)
    return ((n1 + (F32(s1) * d0).astype(F32)).astype(F32) + (F32(s2) * d2).astype(F32)).astype(F32)


def stage(st, x, xe, e0, e1, e2, h1, h2):
    """(x_out, mn) of one stage on flat fp32 arrays"""
    c = KD._Coef(st)
    assert c.guidance == PAIR
    n = e0.size
    with np.errstate(all="ignore"):
        n0, n1, n2 = (np.asarray(KD.to_noise(o, xe, c), dtype=F32) for o in (e0, e1, e2))
        eps = blend(n0, n1, n2, c.cfg_scale, c.cg_scale)
        mn = ((xe - c.sigma_e * eps) / c.alpha_e).astype(F32) if (st.flags & L.F_TO_X0) else eps
        out = KD.combine(c, x, mn, h1, h2, None)     # (model values are fp32: no half differences)
    return np.broadcast_to(out, (n,)).astype(F32), mn


def launch_raw_double(st_ref, b_ref, stream=None):
    """pointer-level double of dpm_stage_launch: a two-condition stage here, every other stage kernel_double's"""
    st, b = st_ref._obj, b_ref._obj
    if st.guidance != PAIR:
        return KD.launch_raw_double(st_ref, b_ref, stream)
    n, B = int(b.n), int(b.batch)
    sd, ed = b.state_dtype, b.eps_dtype
    assert sd != L.DTYPE_F64 and (not b.eps_stride or b.eps_stride == n // B) and not b.x_out2
    assert not (st.flags & (L.F_THRESH | L.F_BLEND | L.F_NOISE | L.F_USER_X0)) and st.form != L.FORM_UNIPC
    x, xe = KD._rd(b.x, n, sd), KD._rd(b.xe, n, sd)
    xe = x if xe is None else xe
    x = xe if x is None else x
    out, mn = stage(st, x, xe, KD._rd(b.e0, n, ed), KD._rd(b.e1, n, ed), KD._rd(b.g, n, ed), KD._rd(b.h1, n, sd),
                    KD._rd(b.h2, n, sd))
    KD._wr(b.x_out, out, sd)
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
    """double of _device._launch_stage (the general loop): two-condition stages here, everything else kernel_double's"""
    if st.guidance != PAIR:
        return KD.launch_stage_double(st, x, xe, e0, e1, g, h1, h2, state_dtype, want_m, ext, opts, coef64)
    assert state_dtype != torch.float64 and not ext
    ref_t = x if x is not None else xe
    ed = e0.dtype
    if ed not in (torch.float32, torch.float16, torch.bfloat16) or (state_dtype != torch.float32 and ed != state_dtype):
        ed = state_dtype
    to = lambda t, dt: None if t is None else (t if t.dtype == dt else t.to(dt))
    flat = lambda t, dt: None if t is None else KD._np(to(t, dt)).reshape(-1)
    xn, xen = flat(x, state_dtype), flat(xe, state_dtype)
    xen = xn if xen is None else xen
    xn = xen if xn is None else xn
    out, mn = stage(st, xn, xen, flat(e0, ed), flat(e1, ed), flat(g, ed), flat(h1, state_dtype), flat(h2, state_dtype))
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(state_dtype).reshape(ref_t.shape)
    store = bool(st.flags & L.F_STORE_M) if want_m is None else want_m
    return conv(out), (conv(mn) if store else None)


def install_pair_double(monkeypatch, S, D):
    """kernel_double.install_cpu_double + the two-condition stage behind every launch entry point"""
    KD.install_cpu_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_launch_stage", launch_stage_double)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw_double)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_double)
