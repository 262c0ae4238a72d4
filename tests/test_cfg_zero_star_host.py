"""CFG-Zero* (dpm_solver_amd.cfg_zero_star, DPM_F_CFG_ZSTAR; C ABI version 216) without a GPU: the helper and the three mutual
refusals, every refusal of the solver, the stage records the binder builds (the kernels replaced by the numpy double,
tests/zstar_double.py), the argument errors dpm_stage_launch decides before it touches HIP -- and that the two older flags'
messages are what they were --, and sample() on the double against a plain numpy walk of the plan."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import kernel_double as KD
import zstar_double as ZD
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule

CFG = L.GUIDE["classifier-free"]


def _net(x, t, c):
    return torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]) + 0.05 * x + 0.2 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]


def _wrapper(model_type="noise", scale=3.0, uncond=True, ns=None):
    ns = ns or make_schedule("sd")
    c = torch.ones(2)
    return D.model_wrapper(_net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=scale, condition=c,
                           unconditional_condition=c * 0 if uncond else None), ns


def _solver(on=True, algorithm_type="dpmsolver++", **kw):
    wkw = {k: kw.pop(k) for k in ("model_type", "scale", "uncond") if k in kw}
    fn, ns = _wrapper(**wkw)
    return D.DPM_Solver(D.cfg_zero_star(fn) if on else fn, ns, algorithm_type=algorithm_type, **kw)


def _x(seed=0):
    return torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------
def test_abi_216_flag_and_binding():
    assert L.lib.dpm_version() >= 216 and L.F_CFG_ZSTAR == 4096
    assert C.sizeof(L.Stage) == L.lib.dpm_sizeof(0) and C.sizeof(L.Buffers) == L.lib.dpm_sizeof(1)
    assert "cfg_zero_star" in D.__all__ and len(L.SYMBOLS) == 62


def test_helper_returns_a_copy_with_the_projection_on():
    fn, _ = _wrapper()
    assert fn.guidance_zero_star is False and fn.zero_star is False
    out = D.cfg_zero_star(fn)
    assert isinstance(out, D.WrappedModel) and out is not fn and out.zero_star is True
    assert fn.guidance_zero_star is False                                    # the original is untouched
    assert out.model is fn.model and out.condition is fn.condition and out.guidance_scale == fn.guidance_scale
    # no classifier-free blend -> nothing to project: the flag is never asked for
    assert D.cfg_zero_star(_wrapper(scale=1.0)[0]).zero_star is False
    assert D.cfg_zero_star(_wrapper(uncond=False)[0]).zero_star is False


def test_helper_refuses_anything_but_a_classifier_free_wrapper():
    ns = make_schedule("sd")
    for bad in (lambda x, t: x, D.model_wrapper(lambda x, t: x, ns), D.model_wrapper(
            lambda x, t: x, ns, guidance_type="classifier", classifier_fn=lambda *a: 0, condition=torch.ones(1))):
        with pytest.raises(ValueError, match="cfg_zero_star: takes the result of model_wrapper\\(..., guidance_type='classifier-free'\\)"):
            D.cfg_zero_star(bad)


def test_the_three_remedies_refuse_each_other():
    fn, _ = _wrapper()
    z = D.cfg_zero_star(fn)
    with pytest.raises(NotImplementedError, match="cfg_zero_star on top of cfg_rescale"):
        D.cfg_zero_star(D.cfg_rescale(fn, 0.7))
    with pytest.raises(NotImplementedError, match="cfg_zero_star on top of cfg_apg"):
        D.cfg_zero_star(D.cfg_apg(fn, 0.5))
    with pytest.raises(NotImplementedError, match="cfg_rescale on top of cfg_zero_star"):
        D.cfg_rescale(z, 0.7)
    with pytest.raises(NotImplementedError, match="cfg_apg on top of cfg_zero_star"):
        D.cfg_apg(z, 0.5)
    # the identities of the two others refuse nothing, in either order
    assert D.cfg_rescale(z, 0.0).zero_star and D.cfg_apg(z, 1.0, 0.0, 0.0).zero_star
    assert D.cfg_zero_star(D.cfg_rescale(fn, 0.0)).zero_star and D.cfg_zero_star(D.cfg_apg(fn, 1.0, 0.0, 0.0)).zero_star


# ------------------------------------------------------------------------------------------------
# the refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    ZD.install_zstar_double(monkeypatch, S, D)
    x = _x()
    dpm = _solver()
    P = "CFG-Zero\\* \\(cfg_zero_star\\).*"
    with pytest.raises(NotImplementedError, match=P + "method='adaptive'"):
        dpm.sample(x, steps=6, order=2, method="adaptive")
    with pytest.raises(NotImplementedError, match=P + "method='adaptive'"):
        dpm.dpm_solver_adaptive(x, 2, 1.0, 1e-3)
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        dpm.sample_sde(x, steps=6, seed=1)
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        dpm.sample_sde_requests([x, x], steps=6, seeds=[1, 2])
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        dpm.sample_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        dpm.sample_unipc_requests([x, x], steps=6)
    with pytest.raises(NotImplementedError, match=P + "slab pool.*no table row kind"):
        dpm.request_pool(slots=8)
    for kw in (dict(rescale=True), dict(apg=True), dict(sde=True)):
        with pytest.raises(NotImplementedError, match=P + "slab pool"):
            dpm.request_pool(slots=8, **kw)
    pool = dpm.request_pool()
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        pool.submit(x, steps=6, sde=True, seed=3)
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        pool.submit_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match=P + "dynamic_thresholding"):
        _solver(correcting_x0_fn="dynamic_thresholding").sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "dynamic_thresholding"):
        _solver(correcting_x0_fn="dynamic_thresholding").data_prediction_fn(x, torch.tensor([0.5]))
    blend = D.MaskBlend(make_schedule("sd"), torch.ones(8, 8), x0=x, noise=x)
    with pytest.raises(NotImplementedError, match=P + "MaskBlend"):
        _solver(correcting_xt_fn=blend).sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "double-precision"):
        dpm.sample(x.double(), steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "double-precision"):
        dpm.sample_requests([x.double(), x.double()], steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "double-precision"):
        dpm.request_pool().submit(x.double(), steps=6)
    fn, ns = _wrapper()
    both = D.cfg_zero_star(fn)
    both.guidance_rescale = 0.7                                              # (set behind the helpers' backs)
    with pytest.raises(NotImplementedError, match=P + "guidance rescale"):
        D.DPM_Solver(both, ns).sample(x, steps=6, order=2)
    both = D.cfg_zero_star(fn)
    both.guidance_apg = (0.5, 0.0, 0.0)
    with pytest.raises(NotImplementedError, match=P + "adaptive projected guidance"):
        D.DPM_Solver(both, ns).sample(x, steps=6, order=2)
    # ... and only where a stage is thresholded: the noise prediction of a thresholding solver involves no thresholding
    assert torch.isfinite(_solver(correcting_x0_fn="dynamic_thresholding").noise_prediction_fn(x, torch.tensor([0.5]))).all()
    # at guidance scale 1 nothing is refused
    _solver(scale=1.0, correcting_x0_fn="dynamic_thresholding").sample(x, steps=4, order=2)
    _solver(scale=1.0).request_pool(slots=8)


# ------------------------------------------------------------------------------------------------
# the records
# ------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """the stage records that reach the launch entry points, as (flags, cfg_scale, cg_scale, guidance) in call order"""
    ZD.install_zstar_double(monkeypatch, S, D)
    seen = []
    raw, multi, stage = S._stage_launch_raw, S._stage_launch_multi_raw, S._launch_stage

    def rec(st):
        seen.append((int(st.flags), float(st.cfg_scale), float(st.cg_scale), int(st.guidance)))

    def raw_spy(st_ref, b_ref, stream):
        rec(st_ref._obj)
        return raw(st_ref, b_ref, stream)

    def multi_spy(st_ref, bufs, n_req, stream):
        per = bool(bufs[0].opts) and bufs[0].opts.contents.per_request_stages == 1
        for r in range(int(n_req)):
            rec(st_ref[r] if per else st_ref._obj)
        return multi(st_ref, bufs, n_req, stream)

    def stage_spy(st, *a, **kw):
        rec(st)
        return stage(st, *a, **kw)
    monkeypatch.setattr(S, "_stage_launch_raw", raw_spy)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", multi_spy)
    monkeypatch.setattr(S, "_launch_stage", stage_spy)
    return seen


RUNS = [dict(steps=6, order=1), dict(steps=6, order=2), dict(steps=6, order=3), dict(steps=6, order=2, method="singlestep"),
        dict(steps=6, order=3, method="singlestep"), dict(steps=6, order=2, method="singlestep_fixed", solver_type="taylor"),
        dict(steps=5, order=1, denoise_to_zero=True)]


@pytest.mark.parametrize("algorithm_type", ["dpmsolver", "dpmsolver++"])
@pytest.mark.parametrize("kw", RUNS, ids=lambda k: "%s%d" % (k.get("method", "multistep"), k["order"]))
def test_flag_reaches_every_classifier_free_record(monkeypatch, algorithm_type, kw):
    seen = _spy(monkeypatch)
    x = _x(1)
    ok = lambda rows: all(f & L.F_CFG_ZSTAR and not f & (L.F_CFG_RESCALE | L.F_CFG_APG) and s == 3.0 and g == CFG
                          for f, s, c, g in rows)
    plain = _solver(False, algorithm_type).sample(x, **kw)
    cgs = [c for f, s, c, g in seen]                                        # cg_scale stays the planner's under the flag
    assert seen and not any(f & L.F_CFG_ZSTAR for f, s, c, g in seen)
    del seen[:]
    dpm = _solver(True, algorithm_type)
    out = dpm.sample(x, **kw)                                               # the prebuilt records (fast path)
    assert ok(seen) and [c for f, s, c, g in seen] == cgs and not torch.equal(out, plain)
    n_fast = len(seen)
    out_i, inter = dpm.sample(x, return_intermediate=True, **kw)            # the general loop binds the same records
    assert len(seen) == 2 * n_fast and ok(seen[n_fast:])
    assert torch.equal(out, out_i) and torch.isfinite(out).all()
    del seen[:]
    outs = dpm.sample_requests([x, x + 1], **kw)                            # one multi-request call per stage
    assert len(seen) == 2 * n_fast and ok(seen)                             # (seen per request)
    assert torch.equal(outs[0], out)
    del seen[:]
    pool = dpm.request_pool()                                               # a RequestPool without slots accepts the solver
    h = [pool.submit(x, **kw), pool.submit(x + 1, **kw)]
    done = {}
    while pool:
        done.update(pool.step())
    assert len(seen) == 2 * n_fast and ok(seen)
    assert torch.equal(done[h[0]], out) and torch.equal(done[h[1]], outs[1])


@pytest.mark.parametrize("how", ["scale1", "no_uncond", "no_helper"])
def test_flag_is_absent_and_every_bit_is_todays(monkeypatch, how):
    seen = _spy(monkeypatch)
    x = _x(2)
    wkw = {"scale1": dict(scale=1.0), "no_uncond": dict(uncond=False)}.get(how, {})
    plain = _solver(False, **wkw).sample(x, steps=6, order=2)
    before = list(seen)
    del seen[:]
    got = _solver(how != "no_helper", **wkw).sample(x, steps=6, order=2)
    assert seen == before and not any(f & L.F_CFG_ZSTAR for f, s, c, g in seen)
    assert torch.equal(got, plain)


def test_switching_the_wrapper_misses_the_cached_records(monkeypatch):
    seen = _spy(monkeypatch)
    x = _x(3)
    dpm = _solver()
    a = dpm.sample(x, steps=4, order=2)
    dpm._wrapped.guidance_zero_star = False
    b = dpm.sample(x, steps=4, order=2)
    half = len(seen) // 2
    assert all(f & L.F_CFG_ZSTAR for f, s, c, g in seen[:half]) and not any(f & L.F_CFG_ZSTAR for f, s, c, g in seen[half:])
    assert not torch.equal(a, b)


def test_split_stage_around_a_callable_x0_corrector_keeps_the_projection(monkeypatch):
    seen = _spy(monkeypatch)
    _solver(correcting_x0_fn=lambda x0, t: x0.clamp(-1, 1)).sample(_x(4), steps=4, order=2)
    pro = [s for s in seen if s[3] == CFG]                                  # the prologue halves carry the blend
    assert pro and all(f & L.F_CFG_ZSTAR for f, s, c, g in pro)
    assert not any(f & L.F_CFG_ZSTAR for f, s, c, g in seen if g != CFG)    # the update halves have no network output


# ------------------------------------------------------------------------------------------------
# sample() on the double against a plain numpy walk of the plan
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("algorithm_type,kw", [("dpmsolver++", dict(steps=6, order=2)), ("dpmsolver", dict(steps=6, order=3)),
                                               ("dpmsolver++", dict(steps=6, order=3, method="singlestep"))],
                         ids=["2M++", "3M", "3S++"])
def test_sample_on_the_double_is_a_numpy_walk_of_the_plan(monkeypatch, model_type, algorithm_type, kw):
    """the plan's stage records, flagged, walked in numpy with zstar_double.stage: buffer roles as the plan names them (state /
    temporary, three history slots).  sample() on the installed double gives the same bits."""
    ZD.install_zstar_double(monkeypatch, S, D)
    x = _x(7)
    dpm = _solver(True, algorithm_type, model_type=model_type)
    got = dpm.sample(x, **kw)
    method = kw.get("method", "multistep")
    plan = dpm._get_plan(method=method, order=kw["order"], steps=kw["steps"], skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=dpm.noise_schedule.T,
                         t_0=1.0 / dpm.noise_schedule.total_N)
    B, n = x.shape[0], x.numel()
    bufs, hist = {0: x.numpy().reshape(-1).copy()}, [None, None, None]
    w = dpm._wrapped
    for ps, (xi, xei, oi) in zip(plan.stages, plan.roles):
        st = dpm._prep_stage(ps.copy())
        assert st.flags & L.F_CFG_ZSTAR
        xs, xe = bufs[xi], bufs[xei]
        xt = torch.from_numpy(xe.reshape(x.shape).copy())
        e0, e1, _ = w.raw_outputs(xt, torch.full((B,), float(st.t_eval)), torch.full((B,), float(st.t_input)))
        out, mn = ZD.stage(st, xs, xe, e0.numpy().reshape(-1), e1.numpy().reshape(-1),
                           hist[st.h1_slot] if st.h1_slot >= 0 else None, hist[st.h2_slot] if st.h2_slot >= 0 else None, B)
        if st.flags & L.F_STORE_M:
            hist[st.m_slot] = mn
        bufs[oi] = out
    assert plan.stages[-1].emits_state
    assert torch.equal(got, torch.from_numpy(bufs[plan.roles[-1][2]].reshape(x.shape)))


# ------------------------------------------------------------------------------------------------
# the C side, before HIP
# ------------------------------------------------------------------------------------------------
def _record(form=L.FORM_TWO, flags=L.F_TO_X0 | L.F_STORE_M | L.F_CFG_ZSTAR, guidance=CFG, cg=4.5, r=0.995, mx=1.0, n=64,
            batch=2, dtype=L.DTYPE_F32):
    """a well-formed flagged request on CPU pointers (never read: the calls below end before any launch)"""
    arena = np.zeros(10 * n * 8 + 64, dtype=np.uint8)
    base = (arena.ctypes.data + 63) // 64 * 64
    st, b = L.Stage(), L.Buffers()
    st.form, st.flags, st.guidance, st.model_type = form, flags, guidance, L.MODEL["noise"]
    st.alpha_e, st.sigma_e, st.cfg_scale, st.cg_scale, st.thr_ratio, st.thr_max = 0.8, 0.6, 7.5, cg, r, mx
    st.cx, st.c0, st.c1 = 0.9, -0.1, 0.05
    st.h1_slot = st.h2_slot = st.m_slot = -1
    p = [base + k * n * 8 for k in range(9)]
    b.x, b.e0, b.e1, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[2], p[3], p[4], p[5], p[6]
    b.n, b.batch, b.state_dtype, b.eps_dtype = n, batch, dtype, dtype
    return st, b, arena


ZS = L.F_TO_X0 | L.F_CFG_ZSTAR
BANNED = "stage_launch: DPM_F_CFG_ZSTAR with guidance rescale, adaptive projected guidance, thresholding, mask blend or noise (flags %d)"
TEXTS = [   # every refusal of the flag, in the order dpm_stage_launch asks: return code and the whole message
    (dict(guidance=L.GUIDE["classifier"]), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_ZSTAR is valid under classifier-free guidance only (guidance 2)"),
    (dict(guidance=L.GUIDE["uncond"]), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_ZSTAR is valid under classifier-free guidance only (guidance 0)"),
    (dict(flags=ZS | L.F_CFG_RESCALE), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_CFG_RESCALE)),
    (dict(flags=ZS | L.F_CFG_APG), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_CFG_APG)),
    (dict(flags=ZS | L.F_THRESH), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_THRESH)),
    (dict(flags=ZS | L.F_BLEND), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_BLEND)),
    (dict(flags=ZS | L.F_NOISE), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_NOISE)),
    (dict(form=L.FORM_UNIPC), L.ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG_ZSTAR on a DPM_FORM_UNIPC stage"),
    (dict(form=6), L.ERR_ARG, "unknown update form 6"),
    (dict(form=-1), L.ERR_ARG, "unknown update form -1"),
    (dict(dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG_ZSTAR with a double state (no double kernel)"),
    (dict(stride=40), L.ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG_ZSTAR with eps_stride=40 (a channel slice of a wider output)"),
    # ... and which of two speaks first: each row fails the check of its own line and every later one it can
    (dict(guidance=0, flags=ZS | L.F_NOISE, form=6, dtype=L.DTYPE_F64, stride=40), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_ZSTAR is valid under classifier-free guidance only (guidance 0)"),
    (dict(flags=ZS | L.F_NOISE, form=6, dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_NOISE)),
    (dict(form=L.FORM_UNIPC, dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG_ZSTAR on a DPM_FORM_UNIPC stage"),
    (dict(form=-1, dtype=L.DTYPE_F64, stride=40), L.ERR_ARG, "unknown update form -1"),
    (dict(dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG_ZSTAR with a double state (no double kernel)"),
    # the new flag together with an old one is reported by the new row, whatever the old flag's own fields hold, with or without
    # DPM_F_TO_X0 (adaptive projected guidance alone asks for it first)
    (dict(flags=L.F_CFG_ZSTAR | L.F_CFG_APG, cg=1.5), L.ERR_UNSUPPORTED, BANNED % (L.F_CFG_ZSTAR | L.F_CFG_APG)),
    (dict(flags=ZS | L.F_CFG_RESCALE, cg=0.0), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_CFG_RESCALE)),
    (dict(flags=ZS | L.F_CFG_RESCALE | L.F_CFG_APG, cg=-1.0), L.ERR_UNSUPPORTED, BANNED % (ZS | L.F_CFG_RESCALE | L.F_CFG_APG)),
]


@pytest.mark.parametrize("kw,code,text", TEXTS, ids=[str(i) for i in range(len(TEXTS))])
def test_every_refusal_has_its_code_its_text_and_its_turn(kw, code, text):
    kw = dict(kw)
    stride = kw.pop("stride", 0)
    st, b, arena = _record(**kw)
    b.eps_stride = stride
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == code
    assert L.lib.dpm_last_error().decode() == text and not arena.any()
    # ... and for a request of a multi-request call, lockstep and with per-request stages, before anything is launched
    ok_st, ok_b, arena2 = _record()
    bs = (L.Buffers * 2)(ok_b, b)
    assert L.lib.dpm_stage_launch_multi(C.byref(st), bs, 2, None) == code
    opts = L.LaunchOpts()
    opts.per_request_stages = 1
    bs[0].opts = C.pointer(opts)
    assert L.lib.dpm_stage_launch_multi((L.Stage * 2)(ok_st, st), bs, 2, None) == code
    assert L.lib.dpm_last_error().decode() == text and not arena.any() and not arena2.any()
    with pytest.raises(ValueError if code == L.ERR_ARG else NotImplementedError):
        L.check(code)


OLD = [   # records WITHOUT the new bit: the two existing flags' messages, to the letter
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE, cg=1.5), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_RESCALE with phi=1.5 (dpm_stage.cg_scale), which is not in (0, 1]"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE, cg=0.7, n=3, batch=3), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_RESCALE needs samples of at least 2 elements (got 1)"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE | L.F_THRESH, cg=0.7), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE with thresholding, mask blend or noise (flags 1033)"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE, cg=0.7, dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE with a double state (no double rescale kernel)"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE, cg=0.7, guidance=2), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_RESCALE is valid under classifier-free guidance only (guidance 2)"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_APG, cg=1.5, r=2.5, mx=0.0), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_APG with eta=1.5 (dpm_stage.cg_scale), which is not in [0, 1]"),
    (dict(flags=L.F_CFG_APG, cg=0.5, r=2.5, mx=0.0), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_APG without DPM_F_TO_X0 (it is defined on the data prediction)"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_APG | L.F_CFG_RESCALE, cg=0.5, r=2.5, mx=0.0), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_APG with guidance rescale, thresholding, mask blend or noise (flags 3073)"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_APG, cg=0.5, r=2.5, mx=0.0, dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_APG with a double state (no double kernel)"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_APG, cg=0.5, r=2.5, mx=0.0, form=L.FORM_UNIPC), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_APG on a DPM_FORM_UNIPC stage"),
]


@pytest.mark.parametrize("kw,code,text", OLD, ids=[str(i) for i in range(len(OLD))])
def test_the_two_existing_flags_keep_their_messages(kw, code, text):
    st, b, arena = _record(**kw)
    assert not st.flags & L.F_CFG_ZSTAR
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == code
    assert L.lib.dpm_last_error().decode() == text and not arena.any()


def test_device_resident_coefficients_are_refused_in_so_many_words():
    """dpm_adaptive_stage_launch hands the stage the ADDRESS of a coefficient record in the handle's device block and refuses
    the flag before anything reads it: zeroed host memory stands in for the handle (no device to create one on)"""
    st, b, arena = _record()
    handle = np.zeros(1 << 16, dtype=np.uint8)
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    assert L.lib.dpm_last_error().decode() == "stage_launch: DPM_F_CFG_ZSTAR with device-resident coefficients"
    assert not arena.any() and not handle.any()
    st.guidance = 0                                     # the record's own errors come first
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_ARG
    assert "classifier-free guidance only" in L.lib.dpm_last_error().decode()


def test_an_empty_batch_is_ok_and_its_record_is_still_checked():
    st, b, _ = _record(n=0, batch=1)
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == 0
    st.guidance = 0
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_ARG


def test_eps_stride_equal_to_the_sample_is_dense():
    st, b, _ = _record(form=L.FORM_UNIPC)               # passes the stride rule ... and fails a later one: the form
    b.eps_stride = b.n // b.batch
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    st.form = 6
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_ARG
    assert "unknown update form 6" in L.lib.dpm_last_error().decode()


def test_table_fill_gives_a_flagged_request_no_row():
    """20 fusable TWO requests, classifier-free: one run of 20 rows.  Flag request 7 and the run has 19 -- in call order,
    without it -- whatever table flags the call carries; DPM_TABLE_FILL launches nothing and never calls HIP."""
    HDR, ROW = L.TABLE_HEADER_BYTES, L.TABLE_ROW_BYTES
    R, N = 20, 2048

    def call(flagged, extra=0):
        st, bs = (L.Stage * R)(), (L.Buffers * R)()
        arena = np.zeros(R * 9 * N * 2 + 64, dtype=np.uint8)
        base = (arena.ctypes.data + 63) // 64 * 64
        for r in range(R):
            s, b = st[r], bs[r]
            s.form, s.flags, s.guidance = L.FORM_TWO, L.F_TO_X0 | L.F_STORE_M, CFG
            s.alpha_e, s.sigma_e, s.cfg_scale, s.cg_scale = 0.8, 0.6, 7.5, 0.7
            if r in flagged:
                s.flags |= L.F_CFG_ZSTAR
            p = [base + (r * 9 + k) * N * 2 for k in range(9)]
            b.x, b.e0, b.e1, b.h1, b.x_out, b.m_out, b.x_out2 = p[0], p[1], p[2], p[3], p[5], p[6], p[7]
            b.n, b.batch, b.state_dtype, b.eps_dtype = N, 2, L.DTYPE_F16, L.DTYPE_F16
        opts = L.LaunchOpts()
        opts.per_request_stages, opts.table_mode = 1, L.TABLE_FILL | extra
        bs[0].opts = C.pointer(opts)
        nbytes = L.table_bytes(R, extra)
        table = np.full(nbytes + 16, 0xAB, dtype=np.uint8)
        off = (-table.ctypes.data) % 16
        bs[0].workspace = table.ctypes.data + off
        assert L.lib.dpm_stage_launch_multi(st, bs, R, None) == 0, L.lib.dpm_last_error()
        body = table[off:off + nbytes]
        rows = lambda k: body[HDR:HDR + k * ROW].reshape(k, ROW)[:, :64].copy().view(np.uint64)
        return body, rows, [int(bs[r].x) for r in range(R)], arena
    for extra in (0, L.TABLE_RESCALE | L.TABLE_APG | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_NOISE):
        body, rows, xs, _a = call((), extra)
        assert [int(v) for v in body[:16].view(np.uint32)] == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
        assert rows(R)[:, 0].tolist() == xs
        body, rows, xs, _a = call({7}, extra)
        assert [int(v) for v in body[:16].view(np.uint32)] == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
        assert rows(R - 1)[:, 0].tolist() == [x for r, x in enumerate(xs) if r != 7]
        assert bool((body[HDR + (R - 1) * ROW:HDR + R * ROW] == 0xAB).all())


# ------------------------------------------------------------------------------------------------
# the double against an independent float64 evaluation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ed", [torch.float32, torch.float16, torch.bfloat16])
def test_double_restates_the_contract_and_its_inputs_are_decidable(ed):
    """the numpy double against a float64 evaluation of the formula (1e-6 of the scale: fp32 roundings only -- nothing is
    rounded to the network's dtype after the loads), and the degenerate sample: S_uu == 0 gives s * o_c"""
    rng = np.random.default_rng(11)
    B, P = 3, 4100
    st, _, _ = _record(form=L.FORM_LIN1, flags=L.F_CFG_ZSTAR)
    rnd = KD.half_rounder(ed) or (lambda a: a)
    e1 = rnd(rng.standard_normal(B * P).astype(np.float32))
    e0 = rnd((0.8 * e1 + 0.6 * rng.standard_normal(B * P)).astype(np.float32))
    x = rng.standard_normal(B * P).astype(np.float32)
    ZD.assert_inputs_decidable(e0, e1, B)
    out, mn = ZD.stage(st, x, x, e0, e1, None, None, B)
    c, u = e0.astype(np.float64).reshape(B, P), e1.astype(np.float64).reshape(B, P)
    a = (c * u).sum(axis=1, keepdims=True) / ((u * u).sum(axis=1, keepdims=True) + 1e-8)
    assert np.all(np.abs(a - 0.8) < 0.05)
    want = (a * u + 7.5 * (c - a * u)).reshape(-1)
    assert float(np.abs(mn - want).max() / np.abs(want).max()) <= 1e-6
    assert np.array_equal(out, (np.float32(0.9) * x - np.float32(-0.1) * mn).astype(np.float32))
    e1[:P] = 0.0
    out2, mn2 = ZD.stage(st, x, x, e0, e1, None, None, B)
    assert np.array_equal(mn2[:P], (np.float32(7.5) * e0[:P]).astype(np.float32)) and np.array_equal(out2[P:], out[P:])
