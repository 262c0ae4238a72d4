"""numpy test double of a Perp-Neg stage (DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 record, include/dpm_hip.h) -- TEST
INFRASTRUCTURE, never imported by the product.  A restatement of the contract on top of kernel_double's `to_noise` / `combine`:

    d0 = o_c - o_u;  d2 = o_n - o_u                       fp32, one rounding each, on the RAW outputs
    S_nd = sum d2 * d0,  S_dd = sum d0 * d0               over the sample, products and sums in double
    a    = fp32(S_nd / S_dd) if S_dd > 0 else 0
    perp = d2 - a * d0;  gd = o_u + s * (d0 - w * perp)    fp32, one rounding per operation; s = cfg_scale, w = cg_scale
    eps  = to_noise(gd, xe); [eps -> x0]; combine (fp32 model values: nothing is rounded to the network's dtype after the
    loads); store

The kernel may add its doubles in any order.  `projection` therefore computes a THREE ways -- a sequential double sum, numpy's
pairwise sum and math.fsum (the exactly rounded sum) -- and `assert_inputs_decidable` fails a test ON THE CPU when the three
disagree in any bit of a for any sample: a precondition on the chosen inputs, under which a correct kernel cannot differ from
this double through summation order.  No sample is skipped.
"""
import math

import numpy as np
import torch

import kernel_double as KD
import pair_double as PD
from dpm_solver_amd import _lib as L

F32, F64 = np.float32, np.float64
PAIR = L.GUIDE["classifier-free-2"]
SUMS = {"seq": lambda a: F64(np.cumsum(a, dtype=F64)[-1]),          # ((a0 + a1) + a2) + ...
        "np": lambda a: F64(np.sum(a, dtype=F64)),                    # pairwise
        "fsum": lambda a: F64(math.fsum(a.tolist()))}                 # exactly rounded


def flagged(st):
    return bool(st.flags & L.F_CFG2_PERP)


def _a(d0, d2, how):
    """a of one sample (the fp32 differences): the products are exact in double"""
    p, q = d0.astype(F64), d2.astype(F64)
    s_dd = SUMS[how](p * p)
    return F32(SUMS[how](q * p) / s_dd) if s_dd > 0 else F32(0)


def differences(oc, ou, on):
    return (oc - ou).astype(F32), (on - ou).astype(F32)


def projection(oc, ou, on, how="seq"):
    """a of every sample: oc, ou, on are [B, P] fp32 arrays; returns B fp32 values"""
    d0, d2 = differences(oc, ou, on)
    return np.array([_a(d0[b], d2[b], how) for b in range(oc.shape[0])], dtype=F32)


def assert_inputs_decidable(e0, e1, e2, batch):
    """the precondition of a bit-exact comparison: a does not depend on the summation order for these inputs (flat fp32 arrays
    of `batch` samples)"""
    oc, ou, on = (e.reshape(batch, -1) for e in (e0, e1, e2))
    fs = {how: projection(oc, ou, on, how) for how in SUMS}
    for how in ("np", "fsum"):
        same = fs[how].view(np.uint32) == fs["seq"].view(np.uint32)
        assert bool(same.all()), "a depends on the summation order for sample %d: %s" % (
            int(np.nonzero(~same)[0][0]), {k: v.tolist() for k, v in fs.items()})


def guided(oc, ou, on, s, w):
    """gd of [B, P] fp32 arrays under the fp32 scales s (guidance) and w (negative)"""
    a = projection(oc, ou, on).reshape(-1, 1)
    d0, d2 = differences(oc, ou, on)
    perp = (d2 - (a * d0).astype(F32)).astype(F32)
    inner = (d0 - (F32(w) * perp).astype(F32)).astype(F32)
    return (ou + (F32(s) * inner).astype(F32)).astype(F32)


def stage(st, x, xe, e0, e1, e2, h1, h2, batch):
    """(x_out, mn) of one flagged stage on flat fp32 arrays"""
    c = KD._Coef(st)
    assert flagged(st) and c.guidance == PAIR
    n = e0.size
    with np.errstate(all="ignore"):
        gd = guided(e0.reshape(batch, -1), e1.reshape(batch, -1), e2.reshape(batch, -1), c.cfg_scale, c.cg_scale).reshape(n)
        eps = KD.to_noise(gd, xe, c)
        mn = ((xe - c.sigma_e * eps) / c.alpha_e).astype(F32) if (st.flags & L.F_TO_X0) else np.asarray(eps, dtype=F32)
        out = KD.combine(c, x, mn, h1, h2, None)     # (model values are fp32: no half differences)
    return np.broadcast_to(out, (n,)).astype(F32), mn


def launch_raw_double(st_ref, b_ref, stream=None, check=True):
    """pointer-level double of dpm_stage_launch: a flagged stage here (the inputs checked decidable unless check=False),
    every other stage pair_double's (which hands on what is not a two-condition stage to kernel_double)"""
    st, b = st_ref._obj, b_ref._obj
    if not flagged(st):
        return PD.launch_raw_double(st_ref, b_ref, stream)
    n, B = int(b.n), int(b.batch)
    sd, ed = b.state_dtype, b.eps_dtype
    assert st.guidance == PAIR and sd != L.DTYPE_F64 and (not b.eps_stride or b.eps_stride == n // B) and not b.x_out2
    assert not (st.flags & (L.F_THRESH | L.F_BLEND | L.F_NOISE | L.F_USER_X0)) and st.form != L.FORM_UNIPC
    x, xe = KD._rd(b.x, n, sd), KD._rd(b.xe, n, sd)
    xe = x if xe is None else xe
    x = xe if x is None else x
    e0, e1, e2 = KD._rd(b.e0, n, ed), KD._rd(b.e1, n, ed), KD._rd(b.g, n, ed)
    if check:
        assert_inputs_decidable(e0, e1, e2, B)
    out, mn = stage(st, x, xe, e0, e1, e2, KD._rd(b.h1, n, sd), KD._rd(b.h2, n, sd), B)
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
    """double of _device._launch_stage (the general loop): flagged stages here, everything else pair_double's"""
    if not flagged(st):
        return PD.launch_stage_double(st, x, xe, e0, e1, g, h1, h2, state_dtype, want_m, ext, opts, coef64)
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
    B = int(ref_t.shape[0])
    e0n, e1n, e2n = flat(e0, ed), flat(e1, ed), flat(g, ed)
    assert_inputs_decidable(e0n, e1n, e2n, B)
    out, mn = stage(st, xn, xen, e0n, e1n, e2n, flat(h1, state_dtype), flat(h2, state_dtype), B)
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(state_dtype).reshape(ref_t.shape)
    store = bool(st.flags & L.F_STORE_M) if want_m is None else want_m
    return conv(out), (conv(mn) if store else None)


def install_perp_double(monkeypatch, S, D):
    """kernel_double.install_cpu_double + the Perp-Neg stage behind every launch entry point"""
    KD.install_cpu_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_launch_stage", launch_stage_double)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw_double)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_double)
