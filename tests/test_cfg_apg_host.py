"""Adaptive projected guidance (dpm_solver_amd.cfg_apg, DPM_F_CFG_APG; C ABI version 214) without a GPU: the helper, every
refusal, the stage records the binder builds and the running average's life (the kernels replaced by the numpy double,
tests/apg_double.py), the argument errors dpm_stage_launch decides before it touches HIP, and sample() / RequestPool on the
double against a 2M loop written out in plain torch float64 (tests/apg_torch_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import apg_double as AD
import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import kernel_double as KD
from apg_torch_ref import ApgModel64, torch_2m_float64
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule

CFG = L.GUIDE["classifier-free"]
APG = (0.5, 2.5, -0.5)          # eta, norm threshold (active at [2,3,8,8]: |d| is about 5), momentum


def _net(x, t, c):
    return torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]) + 0.05 * x


def _wrapper(model_type="noise", scale=3.0, uncond=True, ns=None):
    ns = ns or make_schedule("sd")
    c = torch.ones(2)
    return D.model_wrapper(_net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=scale, condition=c,
                           unconditional_condition=c * 0 if uncond else None), ns


def _solver(apg=APG, algorithm_type="dpmsolver++", **kw):
    wkw = {k: kw.pop(k) for k in ("model_type", "scale", "uncond") if k in kw}
    fn, ns = _wrapper(**wkw)
    return D.DPM_Solver(D.cfg_apg(fn, *apg) if apg is not None else fn, ns, algorithm_type=algorithm_type, **kw)


def _x(seed=0):
    return torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------
def test_abi_214_flag_and_binding():
    assert L.lib.dpm_version() >= 214 and L.F_CFG_APG == 2048
    assert C.sizeof(L.Stage) == L.lib.dpm_sizeof(0) and C.sizeof(L.Buffers) == L.lib.dpm_sizeof(1)
    assert "cfg_apg" in D.__all__


def test_helper_returns_a_copy_with_the_parameters_set():
    fn, _ = _wrapper()
    assert fn.guidance_apg is None and fn.apg is None
    out = D.cfg_apg(fn, 0.25, 10, -0.5)
    assert isinstance(out, D.WrappedModel) and out is not fn and out.apg == (0.25, 10.0, -0.5)
    assert fn.guidance_apg is None                                           # the original is untouched
    assert out.model is fn.model and out.condition is fn.condition and out.guidance_scale == fn.guidance_scale
    assert D.cfg_apg(fn).apg == (0.0, 0.0, 0.0)                              # the defaults: the parallel component removed
    assert D.cfg_apg(fn, np.float32(0.5), 0, 0).apg == (0.5, 0.0, 0.0)
    # no classifier-free blend -> no direction to project: the flag is never asked for
    assert D.cfg_apg(_wrapper(scale=1.0)[0], 0.5).apg is None
    assert D.cfg_apg(_wrapper(uncond=False)[0], 0.5).apg is None


def test_eta_1_without_cap_and_momentum_is_the_identity(monkeypatch):
    AD.install_apg_double(monkeypatch, S, D)
    fn, ns = _wrapper()
    same = D.cfg_apg(fn, 1.0, 0.0, 0.0)
    assert same.guidance_apg is None and same.apg is None
    x = _x(1)
    assert torch.equal(D.DPM_Solver(same, ns).sample(x, steps=4, order=2), D.DPM_Solver(fn, ns).sample(x, steps=4, order=2))
    t = torch.tensor([0.5, 0.5])
    assert torch.equal(same(x, t), fn(x, t))


@pytest.mark.parametrize("args,text", [
    ((-0.1,), "eta must be in"), ((1.5,), "eta must be in"), ((float("nan"),), "eta must be a real number"),
    (("0.5",), "eta must be a real number"), ((None,), "eta must be a real number"), ((True,), "eta must be a real number"),
    ((0.5, -1.0), "norm_threshold must be"), ((0.5, float("inf")), "norm_threshold must be"),
    ((0.5, float("nan")), "norm_threshold must be a real number"), ((0.5, 1j), "norm_threshold must be a real number"),
    ((0.5, 0.0, 1.0), "momentum must be in"), ((0.5, 0.0, -1.0), "momentum must be in"),
    ((0.5, 0.0, float("nan")), "momentum must be a real number"), ((0.5, 0.0, "x"), "momentum must be a real number")])
def test_helper_refuses_arguments_out_of_range(args, text):
    with pytest.raises(ValueError, match=text):
        D.cfg_apg(_wrapper()[0], *args)


def test_helper_refuses_anything_but_a_classifier_free_wrapper():
    ns = make_schedule("sd")
    for bad in (lambda x, t: x, D.model_wrapper(lambda x, t: x, ns), D.model_wrapper(
            lambda x, t: x, ns, guidance_type="classifier", classifier_fn=lambda *a: 0, condition=torch.ones(1))):
        with pytest.raises(ValueError, match="guidance_type='classifier-free'"):
            D.cfg_apg(bad, 0.5)


# ------------------------------------------------------------------------------------------------
# the refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    AD.install_apg_double(monkeypatch, S, D)
    x = _x()
    dpm = _solver()
    P = "adaptive projected guidance.*"
    with pytest.raises(NotImplementedError, match=P + "algorithm_type='dpmsolver'"):
        _solver(algorithm_type="dpmsolver").sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "algorithm_type='dpmsolver'"):
        _solver(algorithm_type="dpmsolver").request_pool().submit(x, steps=6)
    with pytest.raises(NotImplementedError, match=P + "method='adaptive'"):
        dpm.sample(x, steps=6, order=2, method="adaptive")
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        dpm.sample_sde(x, steps=6, seed=1)
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        dpm.sample_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match=P + "slab pool"):
        dpm.request_pool(slots=8)
    pool = dpm.request_pool()
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        pool.submit(x, steps=6, sde=True, seed=3)
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        pool.submit_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match=P + "dynamic_thresholding"):
        _solver(correcting_x0_fn="dynamic_thresholding").sample(x, steps=6, order=2)
    blend = D.MaskBlend(make_schedule("sd"), torch.ones(8, 8), x0=x, noise=x)
    with pytest.raises(NotImplementedError, match=P + "MaskBlend"):
        _solver(correcting_xt_fn=blend).sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "double-precision"):
        dpm.sample(x.double(), steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "double-precision"):
        dpm.sample_requests([x.double(), x.double()], steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "capture with a momentum"):
        dpm.capture(x, steps=6, order=2)
    fn, ns = _wrapper()
    with pytest.raises(NotImplementedError, match="cfg_apg on top of cfg_rescale"):
        D.cfg_apg(D.cfg_rescale(fn, 0.7), 0.5)
    with pytest.raises(NotImplementedError, match="cfg_rescale on top of cfg_apg"):
        D.cfg_rescale(D.cfg_apg(fn, 0.5), 0.7)
    both = D.cfg_apg(fn, 0.5)
    both.guidance_rescale = 0.7                                              # (set behind the helpers' backs)
    with pytest.raises(NotImplementedError, match=P + "guidance rescale"):
        D.DPM_Solver(both, ns).sample(x, steps=6, order=2)
    # the identity refuses nothing
    _solver((1.0, 0.0, 0.0), correcting_x0_fn="dynamic_thresholding").sample(x, steps=4, order=2)
    _solver((1.0, 0.0, 0.0), algorithm_type="dpmsolver").sample(x, steps=4, order=2)


# ------------------------------------------------------------------------------------------------
# the records and the running average
# ------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """the stage records that reach the launch entry points, as (flags, eta, r, beta, guidance, workspace) in call order"""
    AD.install_apg_double(monkeypatch, S, D)
    seen = []
    raw, multi, stage = S._stage_launch_raw, S._stage_launch_multi_raw, S._launch_stage

    def rec(st, ws):
        seen.append((int(st.flags), float(st.cg_scale), float(st.thr_ratio), float(st.thr_max), int(st.guidance), ws))

    def raw_spy(st_ref, b_ref, stream):
        rec(st_ref._obj, int(b_ref._obj.workspace or 0))
        return raw(st_ref, b_ref, stream)

    def multi_spy(st_ref, bufs, n_req, stream):
        per = bool(bufs[0].opts) and bufs[0].opts.contents.per_request_stages == 1
        for r in range(int(n_req)):
            rec(st_ref[r] if per else st_ref._obj, int(bufs[r].workspace or 0))
        return multi(st_ref, bufs, n_req, stream)

    def stage_spy(st, *a, **kw):
        ext = kw.get("ext")
        avg = ext.get("apg_avg") if ext else None
        rec(st, 0 if avg is None else avg.data_ptr())
        return stage(st, *a, **kw)
    monkeypatch.setattr(S, "_stage_launch_raw", raw_spy)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", multi_spy)
    monkeypatch.setattr(S, "_launch_stage", stage_spy)
    return seen


RUNS = [dict(steps=6, order=2), dict(steps=6, order=3), dict(steps=6, order=3, method="singlestep"),
        dict(steps=6, order=2, method="singlestep_fixed", solver_type="taylor"), dict(steps=5, order=1, denoise_to_zero=True)]


@pytest.mark.parametrize("kw", RUNS, ids=lambda k: "%s%d" % (k.get("method", "multistep"), k["order"]))
def test_flag_parameters_and_average_reach_every_record(monkeypatch, kw):
    seen = _spy(monkeypatch)
    x = _x(1)
    want = (float(np.float32(APG[0])), float(np.float32(APG[1])), float(np.float32(APG[2])))
    ok = lambda rows: all(f & L.F_CFG_APG and f & L.F_TO_X0 and (e, r, b) == want and g == CFG and ws for f, e, r, b, g, ws in rows)
    dpm = _solver()
    out = dpm.sample(x, **kw)                                               # the prebuilt records (fast path)
    assert seen and ok(seen) and len({s[5] for s in seen}) == 1             # ONE average per run, on every stage
    n_fast = len(seen)
    out_i, inter = dpm.sample(x, return_intermediate=True, **kw)            # the general loop binds the same records
    assert len(seen) == 2 * n_fast and ok(seen[n_fast:]) and len({s[5] for s in seen[n_fast:]}) == 1
    assert torch.equal(out, out_i) and torch.isfinite(out).all()
    del seen[:]
    outs = dpm.sample_requests([x, x + 1], **kw)                            # one multi-request call per stage
    assert len(seen) == 2 * n_fast and ok(seen) and len({s[5] for s in seen}) == 2      # an average per request
    assert torch.equal(outs[0], out)
    del seen[:]
    pool = dpm.request_pool()                                               # a RequestPool without slots accepts the solver
    h = [pool.submit(x, **kw), pool.submit(x + 1, **kw)]
    done = {}
    while pool:
        done.update(pool.step())
    assert len(seen) == 2 * n_fast and ok(seen)
    assert torch.equal(done[h[0]], out) and torch.equal(done[h[1]], outs[1])


def test_without_momentum_no_average_is_bound(monkeypatch):
    seen = _spy(monkeypatch)
    _solver((0.5, 2.5, 0.0)).sample(_x(1), steps=4, order=2)
    assert seen and all(f & L.F_CFG_APG and b == 0.0 and ws == 0 for f, e, r, b, g, ws in seen)


def test_changing_the_parameters_on_the_wrapper_misses_the_cached_records(monkeypatch):
    seen = _spy(monkeypatch)
    x = _x(3)
    dpm = _solver()
    a = dpm.sample(x, steps=4, order=2)
    dpm._wrapped.guidance_apg = (0.25, 0.0, 0.0)
    b = dpm.sample(x, steps=4, order=2)
    assert {(e, r, bt) for f, e, r, bt, g, ws in seen[len(seen) // 2:]} == {(0.25, 0.0, 0.0)} and not torch.equal(a, b)


def test_split_stage_around_a_callable_x0_corrector_keeps_the_guidance(monkeypatch):
    seen = _spy(monkeypatch)
    _solver(correcting_x0_fn=lambda x0, t: x0.clamp(-1, 1)).sample(_x(4), steps=4, order=2)
    pro = [s for s in seen if s[4] == CFG]                                  # the prologue halves carry the blend
    assert pro and all(s[0] & L.F_CFG_APG and s[5] for s in pro) and len({s[5] for s in pro}) == 1
    assert not any(s[0] & L.F_CFG_APG for s in seen if s[4] != CFG)         # the update halves have no network output


def test_the_average_is_zeroed_between_runs_and_between_pool_requests(monkeypatch):
    AD.install_apg_double(monkeypatch, S, D)
    x = _x(5)
    dpm = _solver()
    kw = dict(steps=5, order=2)
    a = dpm.sample(x, **kw)
    (fr,) = dpm._fast.values()
    assert fr.apg_avg is not None and fr.apg_avg.dtype is torch.float32 and float(fr.apg_avg.abs().max()) > 0   # it was used
    assert torch.equal(dpm.sample(x, **kw), a) and len(dpm._fast) == 1      # the same records, the average zeroed in between
    assert not torch.equal(_solver((APG[0], APG[1], 0.0)).sample(x, **kw), a)            # ... and the momentum matters
    # the general loop and a group of requests start from zero as well
    assert torch.equal(dpm.sample(x, return_intermediate=True, **kw)[0], a)
    assert all(torch.equal(o, a) for o in dpm.sample_requests([x, x], **kw))
    assert all(torch.equal(o, a) for o in dpm.sample_requests([x, x], **kw))
    pool = dpm.request_pool()
    for _ in range(2):                                                      # the second request reuses the first one's records
        h = pool.submit(x, **kw)
        done = {}
        while pool:
            done.update(pool.step())
        assert torch.equal(done[h], a)
    assert len(pool._free) == 1 and len(next(iter(pool._free.values()))) == 1


def test_a_direct_wrapper_call_is_the_first_step_of_a_run(monkeypatch):
    """model_fn / data_prediction_fn / the wrapper's __call__ have no history: a first step, the average zero.  Against the
    model value the first stage of a run stores, at the project's 1e-5 of the scale (torch fp32 against the double)."""
    AD.install_apg_double(monkeypatch, S, D)
    raw = S._stage_launch_raw
    first = []

    def spy(st_ref, b_ref, stream):
        rc = raw(st_ref, b_ref, stream)
        st, b = st_ref._obj, b_ref._obj
        if not first:
            assert st.flags & L.F_STORE_M
            first.append((float(st.t_eval), KD._rd(b.m_out, int(b.n), b.state_dtype)))
        return rc
    monkeypatch.setattr(S, "_stage_launch_raw", spy)
    x = _x(6)
    dpm = _solver()
    dpm.sample(x, steps=4, order=2)
    t_eval, m0 = first[0]
    m0 = torch.from_numpy(m0).reshape(x.shape)
    t = torch.full((2,), t_eval)
    rel = lambda got: float((got - m0).abs().max() / m0.abs().max())
    ns = dpm.noise_schedule
    a, s = ns.marginal_alpha(t).reshape(-1, 1, 1, 1), ns.marginal_std(t).reshape(-1, 1, 1, 1)
    errs = [rel(dpm._wrapped.apg_x0(x, t)), rel(dpm.data_prediction_fn(x, torch.tensor([t_eval]))),
            rel((x - s * dpm._wrapped(x, t)) / a), rel((x - s * dpm.noise_prediction_fn(x, torch.tensor([t_eval]))) / a),
            rel(dpm.model_fn(x, torch.tensor([t_eval])))]
    print("direct calls vs the first stage's model value: %s of the scale" % ["%.3g" % e for e in errs])
    assert max(errs) <= 1e-5
    # ... twice: a direct call leaves no history behind
    assert torch.equal(dpm._wrapped(x, t), dpm._wrapped(x, t))


# ------------------------------------------------------------------------------------------------
# sample() and RequestPool on the double against a plain-torch float64 loop
# ------------------------------------------------------------------------------------------------
def _raw_pair(x, t):
    c = torch.ones(2, dtype=x.dtype)
    return _net(x, t, c), _net(x, t, c * 0)


@pytest.mark.parametrize("model_type", ["noise", "v", "x_start"])
@pytest.mark.parametrize("apg", [APG, (0.0, 0.0, -0.75), (1.0, 2.5, 0.0)], ids=["all", "momentum", "cap"])
def test_sample_and_pool_against_a_plain_torch_float64_2m_loop(monkeypatch, model_type, apg):
    """fp32 states on the numpy double against DPM-Solver++(2M) with the guidance written out in torch float64
    (apg_torch_ref: no planner, no wrapper of the project).  Bar: the project's 1e-5 of the scale."""
    AD.install_apg_double(monkeypatch, S, D)
    ns = make_schedule("sd")
    x = _x(7)
    dpm = _solver(apg, model_type=model_type, scale=3.0)
    want = torch_2m_float64(ApgModel64(_raw_pair, ns, model_type, 3.0, *apg), ns, x, 6)
    got = dpm.sample(x, steps=6, order=2)
    err = float((got.double() - want).abs().max() / want.abs().max())
    pool = dpm.request_pool()
    h = [pool.submit(x, steps=6, order=2), pool.submit(x * 0.5, steps=4, order=1)]
    done = {}
    while pool:
        done.update(pool.step())
    err_p = float((done[h[0]].double() - want).abs().max() / want.abs().max())
    print("cfg_apg 2M %s %s vs a torch float64 loop: sample %.3g, pool %.3g of the scale" % (model_type, apg, err, err_p))
    assert got.dtype is torch.float32 and err <= 1e-5 and err_p <= 1e-5
    assert torch.equal(done[h[0]], got) and torch.equal(done[h[1]], dpm.sample(x * 0.5, steps=4, order=1))
    # the guidance is not a no-op here (eta = 1 with a cap that a sample's direction may stay under is one, up to rounding)
    plain = _solver(None, model_type=model_type, scale=3.0).sample(x, steps=6, order=2)
    assert apg[0] == 1.0 or float((plain - got).abs().max() / want.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------
# the C side, before HIP
# ------------------------------------------------------------------------------------------------
def _record(form=L.FORM_TWO, flags=L.F_TO_X0 | L.F_STORE_M | L.F_CFG_APG, guidance=CFG, eta=0.5, r=2.5, beta=-0.5, n=64, batch=2,
            dtype=L.DTYPE_F32, ws=True):
    """a well-formed flagged request on CPU pointers (never read: the calls below end before any launch)"""
    arena = np.zeros(10 * n * 8 + 64, dtype=np.uint8)
    base = (arena.ctypes.data + 63) // 64 * 64
    st, b = L.Stage(), L.Buffers()
    st.form, st.flags, st.guidance, st.model_type = form, flags, guidance, L.MODEL["noise"]
    st.alpha_e, st.sigma_e, st.cfg_scale, st.cg_scale, st.thr_ratio, st.thr_max = 0.8, 0.6, 7.5, eta, r, beta
    st.cx, st.c0, st.c1 = 0.9, -0.1, 0.05
    st.h1_slot = st.h2_slot = st.m_slot = -1
    p = [base + k * n * 8 for k in range(9)]
    b.x, b.e0, b.e1, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[2], p[3], p[4], p[5], p[6]
    if ws:
        b.workspace = p[7]
    b.n, b.batch, b.state_dtype, b.eps_dtype = n, batch, dtype, dtype
    return st, b, arena


NAN = float("nan")
X0M = L.F_TO_X0 | L.F_STORE_M | L.F_CFG_APG
BAD = [
    (dict(guidance=L.GUIDE["uncond"]), L.ERR_ARG, "classifier-free guidance only"),
    (dict(guidance=L.GUIDE["classifier"]), L.ERR_ARG, "classifier-free guidance only"),
    (dict(eta=1.5), L.ERR_ARG, "not in [0, 1]"),
    (dict(eta=-0.1), L.ERR_ARG, "not in [0, 1]"),
    (dict(eta=NAN), L.ERR_ARG, "not in [0, 1]"),
    (dict(r=-1.0), L.ERR_ARG, "norm threshold"),
    (dict(r=NAN), L.ERR_ARG, "norm threshold"),
    (dict(beta=1.0), L.ERR_ARG, "not in (-1, 1)"),
    (dict(beta=-1.0), L.ERR_ARG, "not in (-1, 1)"),
    (dict(beta=NAN), L.ERR_ARG, "not in (-1, 1)"),
    (dict(ws=False), L.ERR_ARG, "running average in dpm_buffers.workspace"),
    (dict(form=6), L.ERR_ARG, "unknown update form 6"),
    (dict(form=-1), L.ERR_ARG, "unknown update form -1"),
    (dict(flags=L.F_STORE_M | L.F_CFG_APG), L.ERR_UNSUPPORTED, "without DPM_F_TO_X0"),
    (dict(flags=X0M | L.F_CFG_RESCALE), L.ERR_UNSUPPORTED, "guidance rescale, thresholding, mask blend or noise"),
    (dict(flags=X0M | L.F_CFG_RESCALE, eta=0.0), L.ERR_UNSUPPORTED, "guidance rescale, thresholding, mask blend or noise"),
    (dict(flags=X0M | L.F_THRESH), L.ERR_UNSUPPORTED, "guidance rescale, thresholding, mask blend or noise"),
    (dict(flags=X0M | L.F_BLEND), L.ERR_UNSUPPORTED, "guidance rescale, thresholding, mask blend or noise"),
    (dict(flags=X0M | L.F_NOISE), L.ERR_UNSUPPORTED, "guidance rescale, thresholding, mask blend or noise"),
    (dict(form=L.FORM_UNIPC), L.ERR_UNSUPPORTED, "DPM_FORM_UNIPC"),
    (dict(dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, "double state"),
    (dict(stride=40), L.ERR_UNSUPPORTED, "eps_stride"),
]


@pytest.mark.parametrize("kw,code,text", BAD, ids=[t[2][:12].replace(" ", "_") + str(i) for i, t in enumerate(BAD)])
def test_argument_errors_are_decided_before_hip(kw, code, text):
    kw = dict(kw)
    stride = kw.pop("stride", 0)
    st, b, arena = _record(**kw)
    b.eps_stride = stride
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == code
    assert text in L.lib.dpm_last_error().decode()
    # ... and for a request of a multi-request call, lockstep and with per-request stages, before anything is launched
    ok_st, ok_b, arena2 = _record()
    bs = (L.Buffers * 2)(ok_b, b)
    assert L.lib.dpm_stage_launch_multi(C.byref(st), bs, 2, None) == code
    opts = L.LaunchOpts()
    opts.per_request_stages = 1
    bs[0].opts = C.pointer(opts)
    assert L.lib.dpm_stage_launch_multi((L.Stage * 2)(ok_st, st), bs, 2, None) == code
    assert not arena.any() and not arena2.any()                             # no output byte, the running average neither
    with pytest.raises(ValueError if code == L.ERR_ARG else NotImplementedError):
        L.check(code)


PRE = "stage_launch: DPM_F_CFG_APG "
BOTH = X0M | L.F_CFG_RESCALE
TEXTS = [   # every refusal of the flag, in the order dpm_stage_launch asks: return code and the whole message
    (dict(guidance=L.GUIDE["classifier"]), L.ERR_ARG, PRE + "is valid under classifier-free guidance only (guidance 2)"),
    (dict(eta=1.5), L.ERR_ARG, PRE + "with eta=1.5 (dpm_stage.cg_scale), which is not in [0, 1]"),
    (dict(r=-1.0), L.ERR_ARG, PRE + "with a norm threshold of -1 (dpm_stage.thr_ratio), which is not >= 0"),
    (dict(beta=1.0), L.ERR_ARG, PRE + "with a momentum of 1 (dpm_stage.thr_max), which is not in (-1, 1)"),
    (dict(ws=False), L.ERR_ARG, PRE + "with a momentum needs the running average in dpm_buffers.workspace"),
    (dict(form=6), L.ERR_ARG, "unknown update form 6"),
    (dict(flags=L.F_STORE_M | L.F_CFG_APG), L.ERR_UNSUPPORTED, PRE + "without DPM_F_TO_X0 (it is defined on the data prediction)"),
    (dict(flags=X0M | L.F_THRESH), L.ERR_UNSUPPORTED,
     PRE + "with guidance rescale, thresholding, mask blend or noise (flags 2059)"),
    (dict(form=L.FORM_UNIPC), L.ERR_UNSUPPORTED, PRE + "on a DPM_FORM_UNIPC stage"),
    (dict(dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, PRE + "with a double state (no double kernel)"),
    (dict(stride=40), L.ERR_UNSUPPORTED, PRE + "with eps_stride=40 (a channel slice of a wider output)"),
    # both guidance flags: this flag's checks speak, whatever phi / eta is, and none of the other flag's
    (dict(flags=BOTH), L.ERR_UNSUPPORTED, PRE + "with guidance rescale, thresholding, mask blend or noise (flags 3075)"),
    (dict(flags=BOTH, eta=0.0), L.ERR_UNSUPPORTED, PRE + "with guidance rescale, thresholding, mask blend or noise (flags 3075)"),
    (dict(flags=BOTH, eta=1.5), L.ERR_ARG, PRE + "with eta=1.5 (dpm_stage.cg_scale), which is not in [0, 1]"),
    (dict(flags=BOTH, guidance=0), L.ERR_ARG, PRE + "is valid under classifier-free guidance only (guidance 0)"),
    (dict(flags=BOTH & ~L.F_TO_X0), L.ERR_UNSUPPORTED, PRE + "without DPM_F_TO_X0 (it is defined on the data prediction)"),
    # ... and which of two speaks first: each row fails the check of its own line and every later one it can
    (dict(guidance=0, eta=NAN, r=NAN, beta=NAN, ws=False, form=6, flags=L.F_CFG_APG | L.F_NOISE, dtype=L.DTYPE_F64, stride=40),
     L.ERR_ARG, PRE + "is valid under classifier-free guidance only (guidance 0)"),
    (dict(eta=NAN, r=NAN, beta=NAN, ws=False, form=6, flags=L.F_CFG_APG | L.F_NOISE, dtype=L.DTYPE_F64, stride=40),
     L.ERR_ARG, PRE + "with eta=nan (dpm_stage.cg_scale), which is not in [0, 1]"),
    (dict(r=NAN, beta=NAN, ws=False, form=6, flags=L.F_CFG_APG | L.F_NOISE, dtype=L.DTYPE_F64, stride=40),
     L.ERR_ARG, PRE + "with a norm threshold of nan (dpm_stage.thr_ratio), which is not >= 0"),
    (dict(beta=NAN, ws=False, form=6, flags=L.F_CFG_APG | L.F_NOISE, dtype=L.DTYPE_F64, stride=40),
     L.ERR_ARG, PRE + "with a momentum of nan (dpm_stage.thr_max), which is not in (-1, 1)"),
    (dict(ws=False, form=6, flags=L.F_CFG_APG | L.F_NOISE, dtype=L.DTYPE_F64, stride=40),
     L.ERR_ARG, PRE + "with a momentum needs the running average in dpm_buffers.workspace"),
    (dict(form=-1, flags=L.F_CFG_APG | L.F_NOISE, dtype=L.DTYPE_F64, stride=40), L.ERR_ARG, "unknown update form -1"),
    (dict(form=L.FORM_UNIPC, flags=L.F_CFG_APG | L.F_NOISE, dtype=L.DTYPE_F64, stride=40),
     L.ERR_UNSUPPORTED, PRE + "without DPM_F_TO_X0 (it is defined on the data prediction)"),
    (dict(form=L.FORM_UNIPC, flags=X0M | L.F_BLEND, dtype=L.DTYPE_F64, stride=40),
     L.ERR_UNSUPPORTED, PRE + "with guidance rescale, thresholding, mask blend or noise (flags 2083)"),
    (dict(form=L.FORM_UNIPC, dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED, PRE + "on a DPM_FORM_UNIPC stage"),
    (dict(dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED, PRE + "with a double state (no double kernel)"),
]


@pytest.mark.parametrize("kw,code,text", TEXTS, ids=[str(i) for i in range(len(TEXTS))])
def test_every_refusal_keeps_its_code_its_text_and_its_turn(kw, code, text):
    kw = dict(kw)
    stride = kw.pop("stride", 0)
    st, b, arena = _record(**kw)
    b.eps_stride = stride
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == code
    assert L.lib.dpm_last_error().decode() == text and not arena.any()


def test_device_resident_coefficients_are_refused_in_so_many_words():
    """dpm_adaptive_stage_launch hands the stage the ADDRESS of a coefficient record in the handle's device block and refuses
    the flag before anything reads it: zeroed host memory stands in for the handle (no device to create one on), so that the
    address is a small number nobody follows"""
    st, b, arena = _record()
    handle = np.zeros(1 << 16, dtype=np.uint8)
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    assert L.lib.dpm_last_error().decode() == PRE + "with device-resident coefficients"
    assert not arena.any() and not handle.any()
    st.flags |= L.F_CFG_RESCALE                         # the record's own errors come first: here, the two flags together
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    assert L.lib.dpm_last_error().decode() == PRE + "with guidance rescale, thresholding, mask blend or noise (flags 3075)"


def test_an_empty_batch_is_ok_and_its_record_is_still_checked():
    st, b, _ = _record(n=0, batch=1)
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == 0
    st.thr_max = 1.5
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_ARG


def test_a_momentum_in_request_0_of_a_table_call_is_an_argument_error():
    """bs[0].workspace is the table there; the same request at position 1, or without a momentum at 0, fills no row"""
    HDR, ROW = L.TABLE_HEADER_BYTES, L.TABLE_ROW_BYTES
    a = [_record(), _record()]
    st, bs = (L.Stage * 2)(a[0][0], a[1][0]), (L.Buffers * 2)(a[0][1], a[1][1])
    opts = L.LaunchOpts()
    opts.per_request_stages, opts.table_mode = 1, L.TABLE_FILL
    bs[0].opts = C.pointer(opts)
    table = np.full(HDR + 2 * ROW + 16, 0xAB, dtype=np.uint8)
    off = (-table.ctypes.data) % 16
    bs[0].workspace = table.ctypes.data + off
    assert L.lib.dpm_stage_launch_multi(st, bs, 2, None) == L.ERR_ARG
    assert "DPM_F_CFG_APG momentum in st[0]" in L.lib.dpm_last_error().decode() and bool((table == 0xAB).all())
    st[0].thr_max = 0.0
    assert L.lib.dpm_stage_launch_multi(st, bs, 2, None) == 0, L.lib.dpm_last_error()
    body = table[off:off + HDR + 2 * ROW]
    assert [int(v) for v in body[:16].view(np.uint32)] == [L.TABLE_MAGIC, L.lib.dpm_version(), 2, 0]      # no run of rows
    assert bool((body[HDR:] == 0xAB).all())


# ------------------------------------------------------------------------------------------------
# the double against an independent evaluation of the formula
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ed", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("beta", [0.0, -0.5])
def test_double_restates_the_contract_and_its_inputs_are_decidable(ed, beta):
    """the numpy double against a float64 evaluation of the formula (fp32 roundings only: 2e-6 of the scale)"""
    rng = np.random.default_rng(11)
    B, P = 3, 4100
    st, _, _ = _record(form=L.FORM_LIN1, flags=L.F_TO_X0 | L.F_CFG_APG, beta=beta)
    rnd = KD.half_rounder(ed) or (lambda a: a)
    e0, e1 = (rnd(rng.standard_normal(B * P).astype(np.float32)) for _ in range(2))
    x = rng.standard_normal(B * P).astype(np.float32)
    avg = rng.standard_normal(B * P).astype(np.float32) if beta else None
    AD.assert_inputs_decidable(st, x, e0, e1, avg, B)
    out, mn, new_avg = AD.stage(st, x, x, e0, e1, None, None, avg, B)
    f = lambda v: np.float64(np.float32(v))
    X, al, sg = x.astype(np.float64).reshape(B, P), f(0.8), f(0.6)
    c = (X - sg * e0.astype(np.float64).reshape(B, P)) / al
    d = c - (X - sg * e1.astype(np.float64).reshape(B, P)) / al
    if beta:
        d = d + f(beta) * avg.astype(np.float64).reshape(B, P)
        assert float(np.abs(new_avg.reshape(B, P) - d).max() / np.abs(d).max()) <= 1e-6
    sc = np.minimum(1.0, f(2.5) / np.sqrt((d * d).sum(axis=1, keepdims=True)))
    assert (sc < 1).all()                                                   # the cap is active
    par = (sc * (d * c).sum(axis=1, keepdims=True) / (c * c).sum(axis=1, keepdims=True)) * c
    want = (c + (f(7.5) - 1.0) * ((sc * d - par) + f(0.5) * par)).reshape(-1)
    assert float(np.abs(mn - want).max() / np.abs(want).max()) <= 2e-6
    assert np.array_equal(out, (np.float32(0.9) * x - np.float32(-0.1) * mn).astype(np.float32))
    # a degenerate sample (c = 0 everywhere: S_cc = 0): what IEEE gives; the others unaffected
    x[:P] = e0[:P] = np.float32(0.0)
    out2, mn2, _ = AD.stage(st, x, x, e0, e1, None, None, avg, B)
    assert np.isnan(mn2[:P]).all() and np.array_equal(out2[P:], out[P:])
