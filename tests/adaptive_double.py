"""numpy restatements of the device-side adaptive solver (dpm_adaptive_*, csrc/dpm_kernels.hip) -- TEST INFRASTRUCTURE.

  error_double       the error norm of ref :999-1001 in the kernels' arithmetic: fp32 terms, double sum, one rounding, fp32 sqrt
  plan_G, chunk      the two formulas of dpm_adaptive_error's launch: workgroups per sample, elements per workgroup
  controller_double  the loop lines ref :995-1008 in fp32, begin by begin, as adaptive.solve evaluates them
  ulps, check_error, CommitCase
                     the comparisons tests/test_gpu_adaptive_kernels.py applies to the kernels; tests/test_adaptive_double_host.py
                     shows on numpy fakes that each of them can fail
"""
import ctypes as C

import numpy as np
import torch

import guarded as G
from dpm_solver_amd import _lib as L

F32, F64 = np.float32, np.float64
R_ORDER = {2: (0.5, 0.0), 3: (1.0 / 3.0, 2.0 / 3.0)}           # r1, r2 of the higher-order update (ref :976-993)


# ------------------------------------------------------------------------------------------------
# error norm
# ------------------------------------------------------------------------------------------------
def _terms(xl, xh, xp, atol, rtol):
    """the fp32 squares ((xh - xl) / delta)^2 of [batch, per_sample] fp32 arrays"""
    l, h, p = (np.asarray(a, dtype=F32) for a in (xl, xh, xp))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        delta = np.maximum(F32(atol), F32(rtol) * np.maximum(np.abs(l), np.abs(p))).astype(F32)
        v = ((h - l) / delta).astype(F32)
        return (v * v).astype(F32)


def _root(total, n):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt((np.asarray(total, dtype=F64) / F64(n)).astype(F32)).astype(F32)


def batch_max(e):
    """the maximum as atomicMax on the bit patterns of non-negative floats takes it: a NaN is above every number"""
    e = np.asarray(e, dtype=F32)
    return F32(np.nan) if bool(np.isnan(e).any()) else F32(e.max())


def error_double(xl, xh, xp, atol, rtol):
    """(E_b[batch], E_max) as fp32 of [batch, per_sample] arrays -- the arithmetic of kernel_double.adaptive_error_double
    with the per-sample values kept; inf and NaN pass through"""
    sq = _terms(xl, xh, xp, atol, rtol).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = _root(sq.sum(axis=1), sq.shape[1])
    return e, batch_max(e)


def plan_G(batch, per_sample, n_cu):
    """workgroups per sample of dpm_adaptive_error: fill the chip twice, at least 8192 elements each, at most 64"""
    return int(min(64, max(1, min((2 * n_cu + batch - 1) // batch, per_sample // 8192))))


def chunk(per_sample, g):
    """elements per workgroup: the share of a sample rounded up to whole groups of 8"""
    return ((per_sample + g - 1) // g + 7) // 8 * 8


def ulps(a, b):
    """distance of two fp32 numbers in units in the last place (0 for two NaNs or the same infinity; huge when only one of
    them is a NaN)"""
    a, b = F32(a), F32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if (np.isnan(a) and np.isnan(b)) else 2 ** 32
    key = lambda v: (lambda i: i if i >= 0 else -(i & 0x7FFFFFFF))(int(np.array(v, dtype=F32).view(np.int32)))
    return abs(key(a) - key(b))


def check_error(got, want, what=""):
    """an error norm of the kernels against the double's: within 1 fp32 ulp.  The two sum the same non-negative fp32 terms in
    double in different orders: the sums differ by far less than 2^-24 relative, so the one rounding to fp32 moves by at most
    one step and sqrtf keeps that"""
    got, want = np.asarray(got, dtype=F32).reshape(-1), np.asarray(want, dtype=F32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for i in range(got.size):
        d = ulps(got[i], want[i])
        if d > 1:
            raise AssertionError("%s: error norm [%d] = %r, the double gives %r (%d ulps)" % (what, i, got[i], want[i], d))


# ------------------------------------------------------------------------------------------------
# commit: x <- x_higher, x_prev <- x_lower on an accepted step, nothing otherwise
# ------------------------------------------------------------------------------------------------
class CommitCase:
    """the four states of dpm_adaptive_begin in guarded arenas (tests/guarded.py), every payload with bits of its own.  The two
    sources carry TAIL more elements of data behind their n: a copy that runs past n then carries them into a guard of x or
    x_prev (guard bits copied onto guard bits would not show)"""
    NAMES = ("x", "x_prev", "x_lower", "x_higher")
    TAIL = 16

    def __init__(self, dtype, n, offset=0, device="cpu", seed=0, like=None):
        self.dtype, self.n, self.offset, self.device, self.seed = dtype, int(n), offset, device, seed
        es = torch.empty(0, dtype=dtype).element_size()
        g = torch.Generator().manual_seed(7919 * seed + n)
        self.bits, self.arenas = {}, {}
        self.full = {}
        for k in self.NAMES:
            ext = self.n + (self.TAIL if k in ("x_lower", "x_higher") else 0)
            self.full[k] = like.full[k] if like is not None else torch.randn(ext, generator=g).to(dtype).view(G._INT[es])
            self.bits[k] = self.full[k][:self.n]
            self.arenas[k] = G.Arena(dtype, ext, device, offset, bits=self.full[k])

    def on(self, device):
        return CommitCase(self.dtype, self.n, self.offset, device, self.seed, like=self)

    def ptrs(self):
        return [self.arenas[k].ptr for k in self.NAMES]

    def verify(self, accept):
        """accept: x holds the bits of x_higher and x_prev those of x_lower; else all four payloads are as they were.  Always:
        the two sources and every guard untouched"""
        want = {"x": self.bits["x_higher"], "x_prev": self.bits["x_lower"]} if accept else {}
        for k in self.NAMES:
            self.arenas[k].verify("commit %s n=%d offset=%d %s" % (G._name(self.dtype), self.n, self.offset, k), want.get(k))


# ------------------------------------------------------------------------------------------------
# controller
# ------------------------------------------------------------------------------------------------
def _eval(h, what, v):
    a, o = C.c_float(float(v)), C.c_float()
    L.check(L.lib.dpm_schedule_eval(h, what, C.byref(a), 1, C.byref(o)))
    return F32(o.value)


def stage_times(ns_handle, desc, s, t):
    """the three (t_eval, t_input) pairs of the higher-order update s -> t: (s, s1, s1) for order 2, (s, s1, s2) for order 3"""
    order = int(desc.order)
    st = (L.Stage * 3)()
    r1, r2 = R_ORDER[order]
    L.check(L.lib.dpm_coef_singlestep(ns_handle, desc.algorithm_type, desc.solver_type, order, float(s), float(t), r1, r2, 0, st))
    te = [F32(st[i].t_eval) for i in range(order)]
    te += [te[-1]] * (3 - order)
    if L.lib.dpm_schedule_is_discrete(ns_handle):
        inv_n = F32(1.0 / L.lib.dpm_schedule_total_N(ns_handle))
        return [(v, F32(F32(v - inv_n) * F32(1000.0))) for v in te]
    return [(v, v) for v in te]


def t_input_of(ns_handle, t_eval):
    """the fp32 formula of the network's time label applied to one t_eval"""
    if L.lib.dpm_schedule_is_discrete(ns_handle):
        return F32(F32(F32(t_eval) - F32(1.0 / L.lib.dpm_schedule_total_N(ns_handle))) * F32(1000.0))
    return F32(t_eval)


def controller_double(ns_handle, desc, E_script):
    """ref :995-1008 in fp32 -- the arithmetic of adaptive.solve -- as the device runs it: one row per dpm_adaptive_begin.
    Begin 0 follows the reset and decides nothing; begin k + 1 reads E_script[k] (ignored once the run is done).  A NaN
    estimate rejects and ends the run with done = 2; s, h, nfe and the times keep their values.
    Rows: dict(s, t, h, accept, nfe, accepted, iterations, done, times, live) -- the state AFTER the begin; `times` the three
    (t_eval, t_input) pairs the begin wrote (None when it wrote none: the run is done)."""
    order = int(desc.order)
    lam = lambda v: _eval(ns_handle, L.EVAL_LAMBDA, v)
    s, t_0 = F32(desc.t_start), F32(desc.t_end)
    lambda_s, lambda_0 = lam(s), lam(t_0)
    h, t_err, theta = F32(desc.h_init), F32(desc.t_err), F32(desc.theta)
    t = s
    nfe = accepted = 0
    done = int(not (abs(F32(s - t_0)) > t_err))
    rows = []
    for k, E in enumerate([None] + list(E_script)):
        accept = 0
        if k > 0 and not done:
            E = F32(E)
            if np.isnan(E):
                done = 2
            else:
                accept = int(E <= F32(1.0))
                if accept:
                    s = t
                    lambda_s = lam(s)
                with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
                    hn = F32(F32(theta * h) * F32(F64(E) ** (-1.0 / order)))
                room = F32(lambda_0 - lambda_s)
                h = room if room < hn else hn
                nfe += order
                accepted += accept
                if not (abs(F32(s - t_0)) > t_err):
                    done = 1
        times = None
        if not done:
            t = _eval(ns_handle, L.EVAL_INV_LAMBDA, F32(lambda_s + h))
            times = stage_times(ns_handle, desc, s, t)
        rows.append(dict(s=s, t=t, h=h, accept=accept, nfe=nfe, accepted=accepted, iterations=k + 1, done=done, times=times,
                         live=not done))
    return rows
