"""UniPC (DPM_Solver.sample_unipc) -- TEST INFRASTRUCTURE, never imported by the product.

Two independent things:

* `reference_sample` / `reference_scalars`: a float64 restatement of the PUBLISHED UniPC update (Zhao et al. 2023, data
  prediction, orders 1-2, variants bh1 / bh2) in its x-bar form -- predictor and corrector each start from
  xbar_i = (sigma_i / sigma_{i-1}) x_{i-1} - alpha_i expm1(-h) m_{i-1}, the corrector's coefficients come out of
  numpy.linalg.solve -- written from the formulas, not from the planner.  The schedule is handed in as three callables
  (lambda, alpha, sigma of a time, in double).
* `combine_unipc` and the launch doubles: the fp32 numpy double of the DPM_FORM_UNIPC stage (include/dpm_hip.h), one rounding
  per operation, composed with kernel_double.py's prologue and pointer helpers; `install_unipc_double` puts them behind
  every device entry point on top of kernel_double.install_cpu_double.
"""
import numpy as np
import torch

import kernel_double as KD
from dpm_solver_amd import _lib as L

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------
# float64 restatement of the published update
# ------------------------------------------------------------------------------------------------
def step_order(order, i, K, lower_order_final):
    return min(order, i, K + 1 - i) if lower_order_final else min(order, i)


def _bh(variant, hh):
    return hh if variant == "bh1" else np.expm1(hh)


def corrector_rhos(o, hh, B, r):
    """rho^c of a step of order o: [1/2], or the solution of [[1, 1], [r, 1]] rho = [b_1, b_2]"""
    if o == 1:
        return np.array([0.5])
    g1 = np.expm1(hh) / hh - 1.0
    g2 = g1 / hh - 0.5
    return np.linalg.solve(np.array([[1.0, 1.0], [r, 1.0]]), np.array([g1 / B, 2.0 * g2 / B]))


def reference_sample(lam, alpha, sigma, grid, x0_fn, x, order=2, variant="bh2", lower_order_final=True, corrector=True):
    """x_K and the list of the corrected states [x_1 .. x_{K-1}, x_K] in float64.  grid: t_0 .. t_K (floats); x0_fn(x, i): the
    data prediction at grid[i] in float64.  The model is evaluated K times: on x_T and on the predicted states x_1^p ..
    x_{K-1}^p; its value at x_i^p is what enters the history (UniPC does not re-evaluate on the corrected state)."""
    grid = [float(t) for t in grid]
    K = len(grid) - 1
    lm, al, sg = [lam(t) for t in grid], [alpha(t) for t in grid], [sigma(t) for t in grid]
    x = np.asarray(x, dtype=F64)
    m = [x0_fn(x, 0)]
    states = []
    for i in range(1, K + 1):
        o = step_order(order, i, K, lower_order_final)
        h = lm[i] - lm[i - 1]
        hh = -h
        B = _bh(variant, hh)
        xbar = (sg[i] / sg[i - 1]) * x - al[i] * np.expm1(hh) * m[i - 1]
        r = Dp = None
        xp = xbar
        if o == 2:
            r = (lm[i - 2] - lm[i - 1]) / h
            Dp = (m[i - 2] - m[i - 1]) / r
            xp = xbar - al[i] * B * 0.5 * Dp
        if i == K:              # the last step is not corrected
            x = xp
            states.append(x)
            break
        m.append(x0_fn(xp, i))
        if not corrector:
            x = xp
        else:
            rho = corrector_rhos(o, hh, B, r)
            acc = rho[-1] * (m[i] - m[i - 1])
            if o == 2:
                acc = rho[0] * Dp + acc
            x = xbar - al[i] * B * acc
        states.append(x)
    return x, states


def reference_scalars(lam, alpha, sigma, grid, order, variant, lower_order_final):
    """per update stage i = 0 .. K-1 the scalars of include/dpm_hip.h's forms in float64, from the published update:
    predictor of step i+1 (cx, c0 and, second order, k0 = 1 / r0 in FORM_TWO's sign convention and c1) and, for i >= 1, the
    delta-form corrector of step i (c2 = alpha_i B (1/2 - rho_1), k1 = alpha_i B rho_last, k2 = 1 / r), plus the flags"""
    grid = [float(t) for t in grid]
    K = len(grid) - 1
    lm, al, sg = [lam(t) for t in grid], [alpha(t) for t in grid], [sigma(t) for t in grid]
    rows = []
    for i in range(K):
        j = i + 1                                                # the step this stage predicts
        o = step_order(order, j, K, lower_order_final)
        h = lm[j] - lm[j - 1]
        hh = -h
        B = _bh(variant, hh)
        row = dict(p2=o == 2, dp=False, unipc=i >= 1, cx=sg[j] / sg[j - 1], c0=al[j] * np.expm1(hh))
        if o == 2:
            r = (lm[j - 2] - lm[j - 1]) / h                      # D_p = (m_{j-2} - m_{j-1}) / r = k0 (m_{j-1} - m_{j-2})
            row.update(k0=-1.0 / r, c1=al[j] * B * 0.5)
        if i >= 1:                                               # corrector of step i
            oc = step_order(order, i, K, lower_order_final)
            h = lm[i] - lm[i - 1]
            hh = -h
            B = _bh(variant, hh)
            r = (lm[i - 2] - lm[i - 1]) / h if oc == 2 else None
            rho = corrector_rhos(oc, hh, B, r)
            row.update(dp=oc == 2, k1=al[i] * B * rho[-1])
            if oc == 2:
                row.update(c2=al[i] * B * (0.5 - rho[0]), k2=1.0 / r)
        rows.append(row)
    return rows


# ------------------------------------------------------------------------------------------------
# fp32 numpy double of the DPM_FORM_UNIPC stage
# ------------------------------------------------------------------------------------------------
def combine_unipc(st, x, mn, h1, h2):
    """(out, xc) of include/dpm_hip.h's DPM_FORM_UNIPC association, every operation rounded to fp32"""
    c = KD._as_coef(st)
    d1 = mn - h1
    if c.flags & L.F_UNIPC_DP:
        xc = x + (c.c2 * (c.k[2] * (h2 - h1)) - c.k[1] * d1)
    else:
        xc = x - c.k[1] * d1
    if c.flags & L.F_UNIPC_P2:
        out = (c.cx * xc - c.c0 * mn) - c.c1 * (c.k[0] * d1)
    else:
        out = c.cx * xc - c.c0 * mn
    return out.astype(F32), xc.astype(F32)


def launch_raw_double(st_ref, b_ref, stream):
    """pointer-level double of dpm_stage_launch: UniPC stages here, everything else kernel_double's"""
    st, b = st_ref._obj, b_ref._obj
    if st.form != L.FORM_UNIPC:
        return KD.launch_raw_double(st_ref, b_ref, stream)
    n, B, sd, ed = int(b.n), int(b.batch), b.state_dtype, b.eps_dtype
    per = n // B
    assert not (st.flags & (L.F_THRESH | L.F_BLEND | L.F_NOISE)) and (st.flags & L.F_TO_X0) and sd != L.DTYPE_F64

    def eps(ptr):
        if not ptr:
            return None
        if b.eps_stride and b.eps_stride != per:
            full = KD._rd(ptr, (B - 1) * int(b.eps_stride) + per, ed)
            return np.concatenate([full[i * int(b.eps_stride): i * int(b.eps_stride) + per] for i in range(B)])
        return KD._rd(ptr, n, ed)

    x, xe = KD._rd(b.x, n, sd), KD._rd(b.xe, n, sd)
    if xe is None:
        xe = x
    c = KD._Coef(st)
    mn = KD.prologue(c, xe, eps(b.e0), eps(b.e1), KD._rd(b.g, n, ed), KD.half_rounder(ed))
    h2 = KD._rd(b.h2, n, sd) if (st.flags & L.F_UNIPC_DP) else None
    out, xc = combine_unipc(c, x, mn, KD._rd(b.h1, n, sd), h2)
    KD._wr(b.x_out, out, sd)
    if b.x_out2:
        KD._wr(b.x_out2, xc if (st.flags & L.F_STORE_XC) else out, sd)
    if st.flags & L.F_STORE_M:
        KD._wr(b.m_out, mn, sd)
    return 0


def launch_multi_double(st_ref, bufs, n_req, stream):
    for r in range(int(n_req)):
        rc = launch_raw_double(st_ref, KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


def launch_stage_double(st, x, xe, e0, e1, g, h1, h2, state_dtype, want_m=None, ext=None, opts=None, coef64=None):
    """double of _device._launch_stage (the general loop): UniPC stages here, everything else kernel_double's"""
    if st.form != L.FORM_UNIPC:
        return KD.launch_stage_double(st, x, xe, e0, e1, g, h1, h2, state_dtype, want_m, ext, opts, coef64)
    assert state_dtype != torch.float64
    ed = e0.dtype
    if ed not in (torch.float32, torch.float16, torch.bfloat16) or (state_dtype != torch.float32 and ed != state_dtype):
        ed = state_dtype
    to = lambda t, dt: None if t is None else (t if t.dtype == dt else t.to(dt))
    x, xe, h1, h2 = to(x, state_dtype), to(xe, state_dtype), to(h1, state_dtype), to(h2, state_dtype)
    xn = KD._np(x)
    xen = KD._np(xe) if xe is not None else xn
    c = KD._Coef(st)
    mn = KD.prologue(c, xen, KD._np(to(e0, ed)), KD._np(to(e1, ed)), KD._np(to(g, ed)), KD.half_rounder(ed))
    out, xc = combine_unipc(c, xn, mn, KD._np(h1), KD._np(h2))
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(state_dtype).reshape(x.shape)
    x_out = conv(out)
    if ext is not None and ext.get("xc"):
        ext["xc_out"] = conv(xc)
    elif ext is not None and ext.get("dup"):
        ext["x2"] = torch.cat([x_out, x_out])
        x_out = ext["x2"][:x_out.shape[0]]
    store = bool(st.flags & L.F_STORE_M) if want_m is None else want_m
    return x_out, (conv(mn) if store else None)


def install_unipc_double(monkeypatch, S, D):
    """kernel_double.install_cpu_double + the UniPC stage behind every launch entry point"""
    KD.install_cpu_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_launch_stage", launch_stage_double)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw_double)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_double)
