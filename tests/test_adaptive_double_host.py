"""The numpy restatements of the device-side adaptive solver (tests/adaptive_double.py) must be shown to be right, and the
comparisons tests/test_gpu_adaptive_kernels.py applies with them must be shown to fail -- CPU only.

The controller's double replays the three golden adaptive runs from the E sequence the host loop saw; the error norm's double
is held against kernel_double.adaptive_error_double and against a plain float64 evaluation of ref :999-1001; then numpy fakes
with one defect each must be rejected by the same check functions the GPU file uses.
"""
import numpy as np
import pytest
import torch

import adaptive_double as AD
import cases as C
import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import guarded as G
import kernel_double as KD
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule, tt

F32, F64 = np.float32, np.float64
ATOL, RTOL = 0.0078, 0.05


def desc_of(order, algo="dpmsolver", solver="dpmsolver", t_start=1.0, t_end=1e-3, **kw):
    d = L.AdaptiveDesc()
    d.algorithm_type, d.solver_type, d.order = L.ALGO[algo], L.SOLVER[solver], order
    d.model_type, d.guidance, d.guidance_scale = L.MODEL["noise"], L.GUIDE["uncond"], 1.0
    d.t_start, d.t_end, d.h_init, d.atol, d.rtol, d.theta, d.t_err = t_start, t_end, 0.05, ATOL, RTOL, 0.9, 1e-5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("name,sname,order,algo", [("a12", "vp_linear", 2, "dpmsolver"), ("a23", "vp_linear", 3, "dpmsolver"),
                                                   ("a23pp", "sd", 3, "dpmsolver++")])
def test_controller_double_replays_the_golden_runs(golden, capsys, monkeypatch, name, sname, order, algo):
    """the host loop on the CPU double, recording every E it saw, every (s, t) it handed to its lower-order update and every
    lambda_s + h it inverted: controller_double fed that E sequence gives the same s and t bit for bit, the same lambda_s + h
    (the loop's h is visible only through that sum), ends with done = 1 exactly at the loop's last iteration and counts the
    golden NFE"""
    KD.install_cpu_double(monkeypatch, S, D)
    ns = make_schedule(sname)
    dpm = D.DPM_Solver(D.model_wrapper(lambda xx, t: C.model_half(xx, t), ns), ns, algorithm_type=algo)
    dpm.adaptive_on_device = False
    seen_E, seen_st, seen_arg = [], [], []
    err = S._adaptive_error

    def record_E(*a):
        e = err(*a)
        seen_E.append(F32(e.item()))
        return e
    monkeypatch.setattr(S, "_adaptive_error", record_E)
    lower_name = "dpm_solver_first_update" if order == 2 else "singlestep_dpm_solver_second_update"
    lower = getattr(dpm, lower_name)

    def record_st(x, s, t, *a, **kw):
        if kw.get("return_intermediate"):
            seen_st.append((F32(s), F32(t)))
        return lower(x, s, t, *a, **kw)
    monkeypatch.setattr(dpm, lower_name, record_st)
    ev = ns._eval_np

    def record_arg(what, v):
        if what == L.EVAL_INV_LAMBDA:
            seen_arg.append(F32(np.asarray(v).reshape(-1)[0]))
        return ev(what, v)
    monkeypatch.setattr(ns, "_eval_np", record_arg)
    g = lambda k: golden.get("adaptive", "adaptive/%s/%s" % (name, k))
    dpm.sample(tt(g("x"), "cpu"), method="adaptive", order=order, t_end=1e-3)
    assert capsys.readouterr().out.strip() == "adaptive solver nfe %d" % int(g("nfe"))
    assert len(seen_E) == len(seen_st) == int(g("nfe")) // order and len(seen_arg) >= len(seen_E)

    rows = AD.controller_double(ns._h, desc_of(order, algo), seen_E)
    assert len(rows) == len(seen_E) + 1
    bits = lambda v: int(np.array(v, dtype=F32).view(np.int32))
    lam = lambda v: AD._eval(ns._h, L.EVAL_LAMBDA, v)
    for i, (s, t) in enumerate(seen_st):
        r = rows[i]
        assert r["done"] == 0 and r["iterations"] == i + 1
        assert bits(r["s"]) == bits(s) and bits(r["t"]) == bits(t), (i, r["s"], s, r["t"], t)
        assert bits(F32(lam(r["s"]) + r["h"])) == bits(seen_arg[i]), i
        assert r["times"][0][0] == r["s"] and (i == 0 or r["accept"] == int(seen_E[i - 1] <= 1.0))
    assert rows[-1]["done"] == 1 and rows[-1]["nfe"] == int(g("nfe")) and rows[-1]["times"] is None
    assert rows[-1]["accepted"] == sum(int(e <= 1.0) for e in seen_E)


def test_controller_double_edges():
    """E == 1 accepts and its successor rejects; E == 0 and E == +inf move h to the range and to 0; a NaN ends the run with the
    verdict 2 and leaves s, t, h and nfe alone; nothing changes after done"""
    ns = make_schedule("sd")
    d = desc_of(2, "dpmsolver++")
    one, above = F32(1.0), np.nextafter(F32(1.0), F32(2.0))
    r = AD.controller_double(ns._h, d, [one, above, 0.0, 0.5, 0.5, np.nan])
    assert [x["accept"] for x in r] == [0, 1, 0, 1, 1, 0, 0] and [x["done"] for x in r] == [0, 0, 0, 0, 1, 1, 1]
    assert r[6]["nfe"] == r[4]["nfe"] == 8 and r[6]["iterations"] == 7
    lam = lambda v: AD._eval(ns._h, L.EVAL_LAMBDA, v)
    assert r[3]["h"] == F32(lam(F32(d.t_end)) - lam(r[3]["s"])) and r[3]["done"] == 0       # E == 0: capped by the range
    assert r[4]["done"] == 1 and r[4]["times"] is None                                       # ... and that one step arrives
    r = AD.controller_double(ns._h, d, [np.inf, 0.5, 0.5, np.nan, 0.5])
    assert r[1]["h"] == 0 and r[2]["t"] == r[2]["s"] == r[1]["s"] and [x["done"] for x in r] == [0, 0, 0, 0, 2, 2]
    assert r[4]["nfe"] == r[3]["nfe"] == r[5]["nfe"] and r[4]["h"] == r[3]["h"] and r[4]["t"] == r[3]["t"] and r[4]["times"] is None


def _case(batch, per, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    xl = torch.randn((batch, per), generator=g).to(dtype)
    xh = (xl.float() + 0.01 * torch.randn((batch, per), generator=g)).to(dtype)
    xp = torch.randn((batch, per), generator=g).to(dtype)
    return xl, xh, xp


def test_error_double_equals_the_tensor_level_double():
    for i, (batch, per) in enumerate([(1, 1), (3, 7), (2, 255), (5, 2049), (17, 16385)]):
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            xl, xh, xp = _case(batch, per, 11 * i + 1, dtype)
            e, emax = AD.error_double(*(a.float().numpy() for a in (xl, xh, xp)), ATOL, RTOL)
            want = KD.adaptive_error_double(xl, xh, xp, ATOL, RTOL)
            assert e.dtype == F32 and e.shape == (batch,) and emax.dtype == F32
            assert emax.tobytes() == np.array(want.item(), dtype=F32).tobytes() and emax == e.max()


def test_error_double_against_a_float64_evaluation_of_the_reference_lines():
    """ref :999-1001 in float64 on fp32-representable inputs, rounded to fp32 once: within 1 fp32 ulp of error_double.  The
    double sum of non-negative terms adds no error of its own and is rounded once; the roundings of the fp32 terms are
    independent and average out over a sample, and the square root halves what is left"""
    for i, (batch, per) in enumerate([(1, 9), (3, 255), (3, 2048), (2, 16392), (1, 65544)]):
        xl, xh, xp = (a.numpy().astype(F64) for a in _case(batch, per, 5 * i + 2))
        delta = np.maximum(F64(F32(ATOL)), F64(F32(RTOL)) * np.maximum(np.abs(xl), np.abs(xp)))
        want = np.sqrt((((xh - xl) / delta) ** 2).mean(axis=1)).astype(F32)
        e, emax = AD.error_double(xl, xh, xp, ATOL, RTOL)
        AD.check_error(e, want, "float64 evaluation batch=%d per_sample=%d" % (batch, per))
        assert emax == e.max()


def test_error_double_passes_inf_and_nan_through():
    xl, xh, xp = (a.numpy().copy() for a in _case(3, 100, 3))
    xh[1, 5] = 3e38
    e, emax = AD.error_double(xl, xh, xp, ATOL, RTOL)
    assert np.isinf(e[1]) and np.isinf(emax) and np.isfinite(e[[0, 2]]).all()
    xh[2, 99] = np.nan
    e, emax = AD.error_double(xl, xh, xp, ATOL, RTOL)
    assert np.isnan(e[2]) and np.isnan(emax) and np.isinf(e[1])
    AD.check_error(emax, np.nan)
    with pytest.raises(AssertionError):
        AD.check_error(np.inf, np.nan)
    with pytest.raises(AssertionError):
        AD.check_error(3e38, np.inf)
    assert AD.ulps(1.0, np.nextafter(F32(1), F32(2))) == 1 and AD.ulps(0.0, -0.0) == 0 and AD.ulps(np.inf, np.inf) == 0


def test_launch_formulas():
    assert AD.plan_G(1, 16383, 256) == 1 and AD.plan_G(1, 16384, 256) == 2 and AD.plan_G(1, 24584, 256) == 3
    assert AD.plan_G(1, 524288, 256) == 64 and AD.plan_G(1, 532480, 256) == 64 and AD.plan_G(600, 16384, 256) == 1
    assert AD.plan_G(17, 65544, 256) == 8 and AD.plan_G(64, 10 ** 6, 8) == 1
    assert AD.chunk(16384, 2) == 8192 and AD.chunk(16385, 2) == 8200 and AD.chunk(532480, 64) == 8320
    for per in (16384, 16385, 24584, 65544, 532480, 2 ** 22 + 3):
        for g in range(1, min(64, per // 8192) + 1):
            c = AD.chunk(per, g)
            assert c % 8 == 0 and c * g >= per and (g - 1) * c < per          # the last workgroup owns at least one element


# ------------------------------------------------------------------------------------------------
# fakes: one defect each, rejected by the checks of the GPU file
# ------------------------------------------------------------------------------------------------
def _fake_error(xl, xh, xp, g, drop_tail=False, mean_over_chunks=False):
    """the kernel's structure in numpy: g partial sums per sample, added in order"""
    sq = AD._terms(xl, xh, xp, ATOL, RTOL).astype(F64)
    per = sq.shape[1]
    c = AD.chunk(per, g)
    parts = []
    for q in range(g):
        lo, hi = q * c, min(q * c + c, per)
        if drop_tail and q == g - 1:
            hi = lo + (hi - lo) // 8 * 8            # the defect: only whole groups of 8
        parts.append(sq[:, lo:hi].sum(axis=1))
    e = AD._root(sum(parts), c * g if mean_over_chunks else per)
    return e, AD.batch_max(e)


@pytest.mark.parametrize("per,g", [(16385, 2), (24587, 3), (16384, 2), (532480, 64)])
def test_error_check_accepts_the_kernel_structure_and_rejects_the_fakes(per, g):
    xl, xh, xp = (a.numpy() for a in _case(2, per, per))
    want = AD.error_double(xl, xh, xp, ATOL, RTOL)
    good = _fake_error(xl, xh, xp, g)
    AD.check_error(good[0], want[0])
    AD.check_error(good[1], want[1])
    if per % 8:
        with pytest.raises(AssertionError, match="error norm"):
            AD.check_error(_fake_error(xl, xh, xp, g, drop_tail=True)[0], want[0])
    if AD.chunk(per, g) * g > per:
        with pytest.raises(AssertionError, match="error norm"):
            AD.check_error(_fake_error(xl, xh, xp, g, mean_over_chunks=True)[1], want[1])


def _fake_commit(c, accept, defect=None):
    """dpm_adaptive_begin's commit through the arenas' raw pointers"""
    a = c.arenas
    es = a["x"].es
    if accept or defect == "copies_on_reject":
        n = c.n + (16 // es if defect == "one_vector_past_n" else 0)
        G.poke(a["x"].ptr, G.peek(a["x_higher"].ptr, n, es), es)
        G.poke(a["x_prev"].ptr, G.peek(a["x_lower"].ptr, n, es), es)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=G._name)
def test_commit_check_accepts_the_commit_and_rejects_the_fakes(dtype):
    for n, offset in ((1, 0), (9, 1), (2052, 0), (2048, 1)):
        for accept in (True, False):
            c = AD.CommitCase(dtype, n, offset, seed=3)
            _fake_commit(c, accept)
            c.verify(accept)
            with pytest.raises(G.GuardError):
                c.verify(not accept)
        c = AD.CommitCase(dtype, n, offset, seed=4)
        _fake_commit(c, False, "copies_on_reject")
        with pytest.raises(G.GuardError, match="nothing may write it"):
            c.verify(False)
        c = AD.CommitCase(dtype, n, offset, seed=5)
        _fake_commit(c, True, "one_vector_past_n")
        with pytest.raises(G.GuardError, match="guard element overwritten"):
            c.verify(True)
