"""UniPC (DPM_Solver.sample_unipc) without a GPU: the DPM_ALGO_UNIPC plan against a float64 restatement of the published
update, the engine's host code on the fp32 numpy double of the stage, the corrector's gain on an analytic problem, NFE,
argument errors and the lockstep requests."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import unipc_double as UD
from dpm_solver_amd import _lib as L


def _discrete():
    ac = np.cumprod(1 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2).astype(np.float32)
    return D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(ac))


def _schedules():
    return [("discrete", _discrete()), ("linear", D.NoiseScheduleVP("linear"))]


def _eval64(ns, what, t):
    i = np.array([float(t)], dtype=np.float64)
    o = np.empty(1, dtype=np.float64)
    L.check(L.lib.dpm_schedule_eval_f64(ns._h, what, i.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                        o.ctypes.data_as(C.POINTER(C.c_double))))
    return float(o[0])


def _sched64(ns):
    return (lambda t: _eval64(ns, L.EVAL_LAMBDA, t), lambda t: _eval64(ns, L.EVAL_ALPHA, t), lambda t: _eval64(ns, L.EVAL_STD, t))


def _grid(plan):
    n = C.c_int()
    L.check(L.lib.dpm_plan_timesteps(plan.handle, None, 0, C.byref(n)))
    out = (C.c_float * n.value)()
    L.check(L.lib.dpm_plan_timesteps(plan.handle, out, n.value, C.byref(n)))
    return [float(v) for v in out]


def _plan(dpm, ns, steps, order, variant, skip="time_uniform", lof=True, dtz=False, t_T=None, t_0=None):
    return dpm._get_plan(method="multistep", order=order, steps=steps, skip_type=skip, solver_type="dpmsolver",
                         lower_order_final=lof, denoise_to_zero=dtz, t_T=ns.T if t_T is None else t_T,
                         t_0=1. / ns.total_N if t_0 is None else t_0, unipc=variant)


@pytest.mark.parametrize("name,ns", _schedules(), ids=lambda v: v if isinstance(v, str) else "")
def test_plan_scalars_match_the_float64_restatement(name, ns):
    """every scalar field the UniPC plan's forms use, relative 1e-6 (the fp32 rounding of a double is 6e-8; the schedule
    evaluations behind both sides are the same double functions).  Worst seen: 5.9e-8."""
    dpm = D.DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver++")
    lam, alpha, sigma = _sched64(ns)
    worst = 0.0
    for skip in ("time_uniform", "logSNR", "time_quadratic"):
        for order in (1, 2):
            for variant in ("bh1", "bh2"):
                for steps in (2, 3, 5, 20):
                    for lof in (False, True):
                        for dtz in (False, True):
                            if steps < order:
                                continue
                            plan = _plan(dpm, ns, steps, order, variant, skip, lof, dtz)
                            assert plan.unipc and len(plan.stages) == steps + int(dtz)
                            rows = UD.reference_scalars(lam, alpha, sigma, _grid(plan), order, variant, lof)
                            for i, (st, want) in enumerate(zip(plan.stages, rows)):
                                tag = (name, skip, order, variant, steps, lof, i)
                                form = L.FORM_UNIPC if want["unipc"] else (L.FORM_TWO if want["p2"] else L.FORM_LIN1)
                                assert st.form == form and st.index == i and st.emits_state == 1, tag
                                assert bool(st.flags & L.F_UNIPC_P2) == (want["unipc"] and want["p2"]), tag
                                assert bool(st.flags & L.F_UNIPC_DP) == want["dp"], tag
                                assert st.flags & L.F_TO_X0 and not (st.flags & (L.F_THRESH | L.F_NOISE | L.F_STORE_XC)), tag
                                assert bool(st.flags & L.F_STORE_M) == (i + 1 < steps), tag
                                assert (st.h1_slot >= 0) == want["unipc"] and (st.h2_slot >= 0) == want["dp"], tag
                                got = dict(cx=st.cx, c0=st.c0, c1=st.c1, c2=st.c2, k0=st.k[0], k1=st.k[1], k2=st.k[2])
                                for f in ("cx", "c0", "c1", "k0", "c2", "k1", "k2"):
                                    if f in want:
                                        rel = abs(got[f] - want[f]) / abs(want[f])
                                        worst = max(worst, rel)
                                        assert rel <= 1e-6, (tag, f, got[f], want[f])
                            # history slots: a stage reads what the stages one and two before it wrote, and writes elsewhere
                            for i, st in enumerate(plan.stages[:steps]):
                                if st.h1_slot >= 0:
                                    assert st.h1_slot == plan.stages[i - 1].m_slot, (name, skip, steps, i)
                                if st.h2_slot >= 0:
                                    assert st.h2_slot == plan.stages[i - 2].m_slot, (name, skip, steps, i)
                                if st.m_slot >= 0:
                                    assert st.m_slot not in (st.h1_slot, st.h2_slot) and st.m_slot < plan.slots
                            if dtz:
                                assert plan.stages[-1].form == L.FORM_DENOISE
    print("worst relative difference of a plan scalar (%s): %.3g" % (name, worst))


def test_c_planner_rejects_what_has_no_unipc_form():
    ns = _discrete()
    d = L.PlanDesc()
    d.algorithm_type, d.method, d.order, d.steps, d.solver_type = L.ALGO_UNIPC, L.METHOD["multistep"], 3, 10, L.UNIPC_VARIANT["bh2"]
    d.t_start, d.t_end = 1.0, 1e-3
    h = C.c_void_p()
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_ARG
    assert b"follow-up" in L.lib.dpm_last_error()
    d.order, d.solver_type = 2, L.SOLVER["taylor"]
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_ARG
    d.solver_type, d.method = L.UNIPC_VARIANT["bh1"], L.METHOD["singlestep"]
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_UNSUPPORTED
    d.method, d.thresholding = L.METHOD["multistep"], 1
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_UNSUPPORTED
    d.thresholding, d.precision = 0, 1
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_UNSUPPORTED
    st = L.Stage()
    assert L.lib.dpm_coef_first(ns._h, L.ALGO_UNIPC, 1.0, 0.5, C.byref(st)) == L.ERR_ARG
    tp = (C.c_float * 2)(1.0, 0.8)
    assert L.lib.dpm_coef_multistep(ns._h, L.ALGO_UNIPC, 0, 2, tp, 0.5, C.byref(st)) == L.ERR_ARG
    assert L.lib.dpm_version() >= 205


def _x(shape=(2, 4, 8, 8), seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def test_corrector_off_bh2_is_the_multistep_plan_bit_for_bit(monkeypatch):
    UD.install_unipc_double(monkeypatch, S, D)
    ns = _discrete()
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: 0.5 * x + 0.1 * torch.sin(x), ns), ns, algorithm_type="dpmsolver++")
    x = _x()
    for steps in (5, 12, 20):
        for lof in (False, True):
            a = dpm.sample_unipc(x, steps=steps, order=2, variant="bh2", corrector=False, lower_order_final=lof)
            b = dpm.sample(x, steps=steps, order=2, method="multistep", solver_type="dpmsolver", lower_order_final=lof)
            assert torch.equal(a, b)
            assert not torch.equal(a, dpm.sample_unipc(x, steps=steps, order=2, variant="bh2", lower_order_final=lof))


# ---- analytic networks: the raw output as a function of (x, continuous time), written once for torch (fp32) and numpy (double)
def _net(kind, lib):
    if kind == "noise":
        return lambda x, t: x * (0.3 + 0.2 * lib.cos(t))
    if kind == "x_start":
        return lambda x, t: x * (0.5 + 0.1 * t)
    return lambda x, t: x * (0.2 - 0.1 * t) + 0.05 * lib.sin(x)      # "v"


def _x0_double(kind, ns, grid, alpha, sigma, cfg=None):
    """the data prediction at grid[i] in float64 from the analytic network (cfg: (scale, c_uncond, c_cond) factors)"""
    net = _net(kind, np)

    def x0(x, i):
        t = float(grid[i])
        a, s = alpha(t), sigma(t)

        def eps_of(o):
            if kind == "x_start":
                return (x - a * o) / s
            if kind == "v":
                return a * o + s * x
            return o
        if cfg is None:
            eps = eps_of(net(x, t))
        else:
            scale, cu, cc = cfg
            eu, ec = eps_of(cu * net(x, t)), eps_of(cc * net(x, t))
            eps = eu + scale * (ec - eu)
        return (x - s * eps) / a
    return x0


def _engine(kind, ns, cfg=None):
    net = _net(kind, torch)
    cont = (lambda t: t) if ns.schedule != "discrete" else (lambda t: t / 1000. + 1. / ns.total_N)
    tt = lambda t: cont(t).reshape(-1, 1, 1, 1)
    if cfg is None:
        return D.model_wrapper(lambda x, t: net(x, tt(t)), ns, model_type=kind)
    scale, cu, cc = cfg
    B = 2
    return D.model_wrapper(lambda x, t, c: c.reshape(-1, 1, 1, 1) * net(x, tt(t)), ns, model_type=kind,
                           guidance_type="classifier-free", condition=torch.full((B,), cc),
                           unconditional_condition=torch.full((B,), cu), guidance_scale=scale)


END_TO_END = [(k, None) for k in ("noise", "x_start", "v")] + [("noise", (2.5, 0.75, 1.25))]


@pytest.mark.parametrize("name,ns", _schedules(), ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("kind,cfg", END_TO_END, ids=["noise", "x_start", "v", "noise-cfg"])
def test_end_to_end_against_the_float64_restatement(monkeypatch, name, ns, kind, cfg):
    """fp32 states on the numpy double of the stages against the published update in double: <= 1e-5 of the tensor's scale
    (the project's bar), every corrected state and the result.  Step counts 5 .. 20, the range the update was probed in: a
    bar relative to the result's scale presupposes updates whose terms are of that scale.  With 3 steps on the linear
    schedule (t 1 -> 0.667 -> 0.334 -> 0.001) under guidance scale 2.5 the second-order predictor adds terms of magnitude 8,
    6 and 15 to a state of magnitude 1.1: a condition number of ~14 on scalars and operations rounded to 2^-24 each puts the
    floor of ANY fp32 evaluation of that update near 1e-5 (measured there: 1.8e-5, and 5.3e-6 for sample()'s 2M on the same
    grid), so that case says nothing about this code.  Worst measured over the cases below: 1.0e-6 (linear schedule, noise network)."""
    UD.install_unipc_double(monkeypatch, S, D)
    dpm = D.DPM_Solver(_engine(kind, ns, cfg), ns, algorithm_type="dpmsolver++")
    lam, alpha, sigma = _sched64(ns)
    x = _x()
    worst = 0.0
    for variant in ("bh1", "bh2"):
        for order, steps, skip in ((2, 10, "time_uniform"), (2, 20, "logSNR"), (1, 7, "time_quadratic"), (2, 5, "time_uniform")):
            got, inter = dpm.sample_unipc(x, steps=steps, order=order, variant=variant, skip_type=skip, return_intermediate=True)
            assert torch.equal(got, dpm.sample_unipc(x, steps=steps, order=order, variant=variant, skip_type=skip))  # fast loop
            grid = _grid(_plan(dpm, ns, steps, order, variant, skip))
            want, states = UD.reference_sample(lam, alpha, sigma, grid, _x0_double(kind, ns, grid, alpha, sigma, cfg),
                                               x.numpy().astype(np.float64), order, variant)
            assert len(inter) == len(states) == steps
            for g_, w_ in zip(inter + [got], states + [want]):
                err = float(np.max(np.abs(g_.numpy() - w_)) / np.max(np.abs(w_)))
                worst = max(worst, err)
                assert err <= 1e-5, (name, kind, variant, order, steps, skip, err)
    print("worst scale-relative error (%s, %s): %.3g" % (name, kind, worst))


def _gaussian_problem(steps, seed=3):
    """linear VP schedule, per-element Gaussian data x0 ~ N(0, s^2): the exact data prediction and the exact ODE solution"""
    ns = D.NoiseScheduleVP("linear", continuous_beta_0=0.1, continuous_beta_1=20.)
    rng = np.random.default_rng(seed)
    s2 = torch.from_numpy(np.exp(rng.uniform(-2, 1, 4096)).astype(np.float64) ** 2).reshape(1, 4, 32, 32)
    x_T = torch.from_numpy(rng.standard_normal(4096)).reshape(1, 4, 32, 32)
    a = lambda t: _eval64(ns, L.EVAL_ALPHA, t)
    sg = lambda t: _eval64(ns, L.EVAL_STD, t)

    def model(x, t):                                            # E[x0 | x_t] = alpha s^2 x / (alpha^2 s^2 + sigma^2)
        at, st = a(float(t[0])), sg(float(t[0]))
        return ((at * s2 * x.double()) / (at * at * s2 + st * st)).to(x.dtype)
    exact = lambda t: x_T * torch.sqrt(a(t) ** 2 * s2 + sg(t) ** 2) / torch.sqrt(a(1.0) ** 2 * s2 + sg(1.0) ** 2)
    return ns, model, x_T.float(), exact


def test_the_corrector_lowers_the_error_of_2m(monkeypatch):
    """UniPC-2 bh2 against DPM-Solver++ 2M on the same logSNR grid, error against the exact solution of the probability-flow
    ODE for Gaussian data, relative to the solution's scale.  Measured on the CPU double (fp32 states): 20 steps 8.1e-3
    against 1.31e-2 (ratio 0.62), 30 steps 2.6e-3 against 6.2e-3 (ratio 0.42)."""
    UD.install_unipc_double(monkeypatch, S, D)
    for steps in (20, 30):
        ns, model, x_T, exact = _gaussian_problem(steps)
        dpm = D.DPM_Solver(D.model_wrapper(model, ns, model_type="x_start"), ns, algorithm_type="dpmsolver++")
        kw = dict(steps=steps, t_start=1.0, t_end=1e-3, order=2, skip_type="logSNR")
        want = exact(1e-3)
        err = lambda got: float((got.double() - want).abs().max() / want.abs().max())
        e_uni = err(dpm.sample_unipc(x_T, variant="bh2", **kw))
        e_2m = err(dpm.sample(x_T, method="multistep", solver_type="dpmsolver", **kw))
        print("steps %d: err(UniPC-2 bh2) = %.3g, err(2M) = %.3g, ratio %.2f" % (steps, e_uni, e_2m, e_uni / e_2m))
        assert e_uni < e_2m, (steps, e_uni, e_2m)


def test_nfe_is_steps_and_the_network_sees_the_multistep_times(monkeypatch):
    UD.install_unipc_double(monkeypatch, S, D)
    ns = _discrete()
    seen = []

    def model(x, t):
        seen.append(t.clone())
        return 0.5 * x
    dpm = D.DPM_Solver(D.model_wrapper(model, ns), ns, algorithm_type="dpmsolver++")
    x = _x()
    for steps, dtz in ((1, False), (2, False), (7, False), (20, False), (20, True)):
        for order in (1, 2):
            if steps < order:
                continue
            kw = dict(steps=steps, order=order, denoise_to_zero=dtz)
            seen.clear()
            dpm.sample_unipc(x, **kw)
            uni = [t.clone() for t in seen]
            seen.clear()
            dpm.sample(x, method="multistep", **kw)
            assert len(uni) == steps + int(dtz) == len(seen)
            for a, b in zip(uni, seen):
                assert torch.equal(a, b)


def test_errors_come_before_any_device_work():
    ns = _discrete()
    x = torch.zeros(2, 4, 8, 8)                  # a CPU tensor: any device work would raise RuntimeError
    dpm = D.DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver++")
    with pytest.raises(NotImplementedError, match="noise-prediction"):
        D.DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver").sample_unipc(x)
    with pytest.raises(NotImplementedError, match="thresholding"):
        D.DPM_Solver(lambda x, t: x, ns, correcting_x0_fn="dynamic_thresholding").sample_unipc(x)
    with pytest.raises(NotImplementedError, match="callable"):
        D.DPM_Solver(lambda x, t: x, ns, correcting_x0_fn=lambda x0, t: x0).sample_unipc(x)
    with pytest.raises(NotImplementedError, match="correcting_xt_fn"):
        D.DPM_Solver(lambda x, t: x, ns, correcting_xt_fn=lambda x, t, step: x).sample_unipc(x)
    mask = torch.ones(8, 8)
    with pytest.raises(NotImplementedError, match="correcting_xt_fn"):
        D.DPM_Solver(lambda x, t: x, ns, correcting_xt_fn=D.MaskBlend(ns, mask, x, noise=x)).sample_unipc(x)
    with pytest.raises(NotImplementedError, match="double"):
        dpm.sample_unipc(x.double())
    with pytest.raises(ValueError, match="'order' must be 1 or 2.*follow-up"):
        dpm.sample_unipc(x, order=3)
    with pytest.raises(ValueError, match="'order' must be 1 or 2"):
        dpm.sample_unipc(x, order=0)
    with pytest.raises(ValueError, match="'variant' must be either 'bh1' or 'bh2'"):
        dpm.sample_unipc(x, variant="vary_coeff")
    with pytest.raises(ValueError, match="skip_type"):
        dpm.sample_unipc(x, skip_type="nope")
    with pytest.raises(AssertionError):
        dpm.sample_unipc(x, steps=1, order=2)
    with pytest.raises(NotImplementedError, match="UniPC"):
        dpm.request_pool().submit(x, unipc="bh2")
    for fn in (dpm.sample_unipc, lambda x, **kw: dpm.sample_unipc_requests([x, x], **kw)):
        with pytest.raises(ValueError, match="variant"):
            fn(x, variant="bh3")
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # ... and the checks pass: the device is required
        dpm.sample_unipc(x)


def test_requests_equal_the_per_request_calls(monkeypatch):
    UD.install_unipc_double(monkeypatch, S, D)
    ns = _discrete()
    launches = []
    real = S._stage_launch_multi_raw
    monkeypatch.setattr(S, "_stage_launch_multi_raw", lambda st, a, n, s: (launches.append(int(n)), real(st, a, n, s))[1])
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: 0.5 * x + 0.1 * torch.cos(x), ns), ns, algorithm_type="dpmsolver++")
    xs = [_x(seed=i) for i in range(5)]
    for kw in (dict(steps=6), dict(steps=9, order=1, variant="bh1"), dict(steps=5, denoise_to_zero=True, skip_type="logSNR")):
        launches.clear()
        got = dpm.sample_unipc_requests(xs, **kw)
        assert launches == [5] * (kw["steps"] + int(kw.get("denoise_to_zero", False)))      # one fused launch per stage
        for g_, x in zip(got, xs):
            assert torch.equal(g_, dpm.sample_unipc(x, **kw))
    # the fall-backs: one request, differing shapes, return_intermediate, corrector off
    launches.clear()
    assert torch.equal(dpm.sample_unipc_requests(xs[:1], steps=6)[0], dpm.sample_unipc(xs[0], steps=6))
    mixed = [xs[0], _x((1, 4, 8, 8), 9)]
    for g_, x in zip(dpm.sample_unipc_requests(mixed, steps=6), mixed):
        assert torch.equal(g_, dpm.sample_unipc(x, steps=6))
    for (g_, gi), x in zip(dpm.sample_unipc_requests(xs[:2], steps=6, return_intermediate=True), xs):
        w_, wi = dpm.sample_unipc(x, steps=6, return_intermediate=True)
        assert torch.equal(g_, w_) and len(gi) == len(wi) == 6 and all(torch.equal(a, b) for a, b in zip(gi, wi))
    assert launches == []
    for g_, x in zip(dpm.sample_unipc_requests(xs[:3], steps=6, corrector=False), xs):
        assert torch.equal(g_, dpm.sample(x, steps=6))
