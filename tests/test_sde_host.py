"""SDE-DPM-Solver++ (DPM_Solver.sample_sde) without a GPU: the noise generator's integer stream, the SDE plan against the ODE
multistep plan and a float64 restatement of its scalars, the argument errors, and the seed rules on the CPU double."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import sde_double as SD
from dpm_solver_amd import _lib as L


def test_philox_known_answer_vectors():
    m = 0xFFFFFFFF
    assert ["%08x" % int(v) for v in SD.philox4x32_10((0, 0, 0, 0), (0, 0))] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert ["%08x" % int(v) for v in SD.philox4x32_10((m, m, m, m), (m, m))] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_noise_restatement_is_standard_normal():
    z = SD.noise_z64(12345, 7, 1 << 18)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)
    u = SD.unit(np.array([0, 0xFFFFFFFF], dtype=np.uint64))
    assert 0 < u[0] < u[1] < 1 and np.float32(u[1]) == u[1]


def _schedules():
    ac = np.cumprod(1 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2).astype(np.float32)
    return [("discrete", D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(ac))),
            ("linear", D.NoiseScheduleVP("linear")), ("cosine", D.LegacyNoiseScheduleVP("cosine"))]


def _eval64(ns, what, t):
    i = np.array([float(t)], dtype=np.float64)
    o = np.empty(1, dtype=np.float64)
    L.check(L.lib.dpm_schedule_eval_f64(ns._h, what, i.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                        o.ctypes.data_as(C.POINTER(C.c_double))))
    return float(o[0])


def _ulps(a, b):
    return abs(float(a) - float(b)) / float(np.spacing(np.float32(abs(b)) if b != 0 else np.float32(1e-30)))


@pytest.mark.parametrize("name,ns", _schedules(), ids=lambda v: v if isinstance(v, str) else "")
def test_sde_plan_is_the_multistep_plan_with_sde_scalars(name, ns):
    dpm = D.DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver++")
    t_0, t_T = 1. / ns.total_N, ns.T
    for skip in ("time_uniform", "logSNR", "time_quadratic"):
        for order in (1, 2):
            for solver in ("dpmsolver", "taylor"):
                for lof in (False, True):
                    for dtz in (False, True):
                        kw = dict(method="multistep", order=order, steps=7, skip_type=skip, solver_type=solver,
                                  lower_order_final=lof, denoise_to_zero=dtz, t_T=t_T, t_0=t_0)
                        ode, sde = dpm._get_plan(**kw), dpm._get_plan(sde=True, **kw)
                        assert sde.sde and not ode.sde and len(sde.stages) == len(ode.stages) and sde.slots == ode.slots
                        assert sde.roles == ode.roles
                        for a, b in zip(ode.stages, sde.stages):
                            for f in ("index", "form", "model_type", "guidance", "outer_step", "emits_state", "x_src",
                                      "xe_src", "h1_slot", "h2_slot", "m_slot", "t_eval", "t_input", "t_out", "alpha_e",
                                      "sigma_e"):
                                assert getattr(a, f) == getattr(b, f), f
                            if b.form == L.FORM_DENOISE:
                                assert b.flags == a.flags and not (b.flags & L.F_NOISE) and b.c2 == a.c2
                                continue
                            assert b.flags == a.flags | L.F_NOISE
                            ts, tt = float(b.t_eval), float(b.t_out)
                            lam = lambda t: _eval64(ns, L.EVAL_LAMBDA, t)
                            h = lam(tt) - lam(ts)
                            a_t, s_t, s_s = _eval64(ns, L.EVAL_ALPHA, tt), _eval64(ns, L.EVAL_STD, tt), _eval64(ns, L.EVAL_STD, ts)
                            em = np.expm1(-2 * h)
                            want = dict(cx=s_t / s_s * np.exp(-h), c0=a_t * em, c2=s_t * np.sqrt(-em))
                            if b.form == L.FORM_TWO:
                                tp = float(sde.stages[b.index - 1].t_eval)
                                want["k0"] = h / (lam(ts) - lam(tp))
                                want["c1"] = 0.5 * a_t * em if solver == "dpmsolver" else -a_t * (1 + em / (2 * h))
                            for f, v in want.items():
                                got = b.k[0] if f == "k0" else getattr(b, f)
                                assert _ulps(got, v) <= 2, (name, skip, order, solver, f, got, v)


def test_errors_come_before_any_device_work():
    ns = _schedules()[0][1]
    x = torch.zeros(2, 4, 8, 8)                  # a CPU tensor: any device work would raise RuntimeError
    dpm = D.DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver++")
    with pytest.raises(NotImplementedError, match="noise-prediction"):
        D.DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver").sample_sde(x)
    with pytest.raises(NotImplementedError, match="thresholding"):
        D.DPM_Solver(lambda x, t: x, ns, correcting_x0_fn="dynamic_thresholding").sample_sde(x)
    with pytest.raises(NotImplementedError, match="callable"):
        D.DPM_Solver(lambda x, t: x, ns, correcting_x0_fn=lambda x0, t: x0).sample_sde(x)
    with pytest.raises(ValueError, match="'order' must be 1 or 2"):
        dpm.sample_sde(x, order=3)
    with pytest.raises(ValueError, match="not both"):
        dpm.sample_sde(x, seed=1, generator=torch.Generator())
    for bad in (-1, 1 << 64, 1.5):
        with pytest.raises(ValueError):
            dpm.sample_sde(x, seed=bad)
    with pytest.raises(NotImplementedError, match="double"):
        dpm.sample_sde(x.double(), seed=1)
    with pytest.raises(ValueError, match="skip_type"):
        dpm.sample_sde(x, seed=1, skip_type="nope")
    with pytest.raises(ValueError, match="solver_type"):
        dpm.sample_sde(x, seed=1, solver_type="nope")
    with pytest.raises(AssertionError):
        dpm.sample_sde(x, seed=1, steps=1, order=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # ... and the checks pass: the device is required
        dpm.sample_sde(x, seed=1)


def test_c_planner_rejects_what_has_no_sde_form():
    ns = _schedules()[0][1]
    d = L.PlanDesc()
    d.algorithm_type, d.method, d.order, d.steps = L.ALGO_SDE_DPMSOLVERPP, L.METHOD["multistep"], 3, 10
    d.t_start, d.t_end = 1.0, 1e-3
    h = C.c_void_p()
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_ARG
    d.order, d.method = 2, L.METHOD["singlestep"]
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_UNSUPPORTED
    d.method, d.thresholding = L.METHOD["multistep"], 1
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_UNSUPPORTED
    st = L.Stage()
    assert L.lib.dpm_coef_first(ns._h, L.ALGO_SDE_DPMSOLVERPP, 1.0, 0.5, C.byref(st)) == L.ERR_ARG


def _run(monkeypatch, **kw):
    ns = _schedules()[0][1]
    SD.install_sde_double(monkeypatch, S, D)
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: 0.5 * x, ns), ns, algorithm_type="dpmsolver++")
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 4, 8, 8)).astype(np.float32))
    return dpm, x


def test_seed_rules_on_the_cpu_double(monkeypatch):
    dpm, x = _run(monkeypatch)
    run = lambda **kw: dpm.sample_sde(x, steps=6, **kw)
    a, b, a2 = run(seed=5), run(seed=6), run(seed=5)
    assert torch.equal(a, a2) and not torch.equal(a, b)                       # launch records do not cache the seed
    ode = dpm.sample(x, steps=6)
    assert not torch.equal(a, ode)
    g_seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64,
                               generator=torch.Generator().manual_seed(3)).item()) % (1 << 64)
    assert torch.equal(run(generator=torch.Generator().manual_seed(3)), run(seed=g_seed))
    torch.manual_seed(11)
    c = run()
    torch.manual_seed(11)
    assert torch.equal(run(), c)
    assert torch.equal(run(seed=(1 << 64) - 1), run(seed=(1 << 64) - 1))


def test_double_adds_exactly_the_scaled_restated_noise(monkeypatch):
    """one first-order SDE stage on the double = the ODE-form update with the SDE scalars + c2 * z of the restatement"""
    dpm, x = _run(monkeypatch)
    out = dpm.sample_sde(x, steps=1, order=1, seed=77)
    plan = dpm._get_plan(method="multistep", order=1, steps=1, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1. / 1000, sde=True)
    st = plan.stages[0]
    xn = x.numpy().reshape(-1)
    eps = np.float32(0.5) * xn
    x0 = ((xn - np.float32(st.sigma_e) * eps) / np.float32(st.alpha_e)).astype(np.float32)
    upd = (np.float32(st.cx) * xn - np.float32(st.c0) * x0).astype(np.float32)
    z = SD.noise_z64(77, 0, xn.size).astype(np.float32)
    want = (upd + (np.float32(st.c2) * z).astype(np.float32)).astype(np.float32)
    assert np.array_equal(out.numpy().reshape(-1), want)
