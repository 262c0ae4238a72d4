"""Guidance over two conditions (dpm_solver_amd.cfg_pair, DPM_GUIDE_CFG2; C ABI version 218) without a GPU: the helper and its
two (s1, s2) mappings, the identity settings, every refusal, the stage records the binder builds (the kernels replaced by the
numpy double, tests/pair_double.py), the argument errors dpm_stage_launch decides before it touches HIP, the planner, the cache
keys, and sample() on the double against a torch float64 statement of the three-branch blend."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import kernel_double as KD
import pair_double as PD
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule

CFG, PAIR = L.GUIDE["classifier-free"], L.GUIDE["classifier-free-2"]
F32 = np.float32


class Net:
    """a network whose output depends on x, t and the per-sample condition; records the batch and conditions of every call"""

    def __init__(self):
        self.calls = []

    def __call__(self, x, t, c):
        self.calls.append((int(x.shape[0]), c.detach().clone()))
        cc = c.reshape(-1, 1, 1, 1).to(x.dtype)
        return torch.tanh(x * 0.7) * (0.5 + 0.1 * cc) + 0.05 * x + 0.2 * cc + 0.01 * t.reshape(-1, 1, 1, 1).to(x.dtype)


def _wrapper(model_type="noise", scale=3.0, uncond=True, net=None, ns=None):
    ns = ns or make_schedule("sd")
    c = torch.ones(2)
    return D.model_wrapper(net or Net(), ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=scale,
                           condition=c, unconditional_condition=c * 0 if uncond else None), ns


C2 = torch.full((2,), -0.5)


def _solver(scale2=1.5, nested=False, algorithm_type="dpmsolver++", **kw):
    wkw = {k: kw.pop(k) for k in ("model_type", "scale", "net") if k in kw}
    fn, ns = _wrapper(**wkw)
    return D.DPM_Solver(fn if scale2 is None else D.cfg_pair(fn, C2, scale2, nested), ns, algorithm_type=algorithm_type, **kw)


def _x(seed=0):
    return torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------
def test_abi_218_value_and_binding():
    assert L.lib.dpm_version() >= 218 and PAIR == 3
    assert C.sizeof(L.Stage) == L.lib.dpm_sizeof(0) and C.sizeof(L.Buffers) == L.lib.dpm_sizeof(1)
    assert "cfg_pair" in D.__all__ and len(L.SYMBOLS) == 62           # no struct grew, no entry point was added


def test_helper_returns_a_copy_with_the_pair_set():
    fn, _ = _wrapper()
    assert fn.guidance_pair is None and fn.pair is None and fn.effective_guidance == "classifier-free"
    out = D.cfg_pair(fn, C2, 1.5)
    assert isinstance(out, D.WrappedModel) and out is not fn and fn.guidance_pair is None      # the original is untouched
    assert out.model is fn.model and out.condition is fn.condition and out.guidance_scale == fn.guidance_scale
    assert out.pair[0] is C2 and out.pair[1:] == (3.0, 1.5) and out.effective_guidance == "classifier-free-2"
    # the second condition still guides at guidance_scale == 1
    one = D.cfg_pair(_wrapper(scale=1.0)[0], C2, 1.5)
    assert one.effective_guidance == "classifier-free-2" and one.pair[1:] == (1.0, 1.5)


def test_both_mappings():
    fn, _ = _wrapper(scale=7.5)
    assert D.cfg_pair(fn, C2, 1.5).pair[1:] == (7.5, 1.5)                               # composable: s1 = s, s2 = scale2
    assert D.cfg_pair(fn, C2, 1.5, nested=True).pair[1:] == (7.5, 1.5 - 7.5)            # nested: s2 = scale2 - s, in double
    assert D.cfg_pair(_wrapper(scale=0.1)[0], C2, 0.3, nested=True).pair[2] == 0.3 - 0.1   # (not fp32(0.3) - fp32(0.1))


def test_identity_settings_are_a_plain_copy_and_evaluate_no_third_branch(monkeypatch):
    PD.install_pair_double(monkeypatch, S, D)
    x = _x(1)
    net = Net()
    plain = _solver(None, net=net).sample(x, steps=4, order=2)
    n_plain = list(net.calls)
    for scale2, nested in ((0.0, False), (3.0, True), (-0.0, False)):
        net = Net()
        dpm = _solver(scale2, nested, net=net)
        w = dpm._wrapped
        assert w.pair is None and w.guidance_pair is None and w.effective_guidance == "classifier-free"
        assert torch.equal(dpm.sample(x, steps=4, order=2), plain)
        assert [b for b, _ in net.calls] == [b for b, _ in n_plain] == [4] * len(net.calls)     # 2B, never 3B


def test_helper_validation():
    ns = make_schedule("sd")
    for bad in (lambda x, t: x, D.model_wrapper(lambda x, t: x, ns), D.model_wrapper(
            lambda x, t: x, ns, guidance_type="classifier", classifier_fn=lambda *a: 0, condition=torch.ones(1))):
        with pytest.raises(ValueError, match="cfg_pair: takes the result of model_wrapper\\(..., guidance_type='classifier-free'\\)"):
            D.cfg_pair(bad, C2, 1.0)
    with pytest.raises(ValueError, match="cfg_pair: takes a classifier-free wrapper with an unconditional_condition"):
        D.cfg_pair(_wrapper(uncond=False)[0], C2, 1.0)
    fn, _ = _wrapper()
    for bad in (float("nan"), float("inf"), -float("inf"), True, "1.5", None):
        with pytest.raises(ValueError, match="cfg_pair: scale2 must be a finite real number"):
            D.cfg_pair(fn, C2, bad)
    with pytest.raises(ValueError, match="cfg_pair: condition2 must be a tensor"):
        D.cfg_pair(fn, [0.0, 0.0], 1.0)
    with pytest.raises(ValueError, match="cfg_pair: condition2 has shape \\(3,\\)"):
        D.cfg_pair(fn, torch.zeros(3), 1.0)
    with pytest.raises(ValueError, match="cfg_pair: nested must be a bool"):
        D.cfg_pair(fn, C2, 1.0, nested=1)
    with pytest.raises(ValueError, match="cfg_pair: the wrapper's guidance_scale must be a finite real number"):
        D.cfg_pair(_wrapper(scale=float("nan"))[0], C2, 1.0)


def test_pair_and_remedies_refuse_each_other_in_either_order():
    fn, _ = _wrapper()
    p = D.cfg_pair(fn, C2, 1.5)
    for name, make in (("cfg_rescale", lambda f: D.cfg_rescale(f, 0.7)), ("cfg_apg", lambda f: D.cfg_apg(f, 0.5)),
                       ("cfg_zero_star", D.cfg_zero_star)):
        with pytest.raises(NotImplementedError, match="cfg_pair on top of %s" % name):
            D.cfg_pair(make(fn), C2, 1.5)
        with pytest.raises(NotImplementedError, match="%s on top of cfg_pair" % name):
            make(p)
    # the identities of the remedies refuse nothing, in either order
    assert D.cfg_rescale(p, 0.0).pair is not None and D.cfg_apg(p, 1.0, 0.0, 0.0).pair is not None
    assert D.cfg_pair(D.cfg_rescale(fn, 0.0), C2, 1.5).pair is not None


def test_raw_outputs_is_one_call_on_three_copies_in_the_contracts_order():
    net = Net()
    fn = D.cfg_pair(_wrapper(net=net)[0], C2, 1.5)
    x = _x(2)
    t = torch.full((2,), 0.5)
    e0, e1, e2 = fn.raw_outputs(x, t)
    assert len(net.calls) == 1 and net.calls[0][0] == 6
    assert torch.equal(net.calls[0][1], torch.cat([torch.zeros(2), torch.ones(2), C2]))      # (uncond, condition, condition2)
    ti = fn.get_model_input_time(t)
    lone = Net()
    assert torch.equal(e0, lone(x, ti, torch.ones(2))) and torch.equal(e1, lone(x, ti, torch.zeros(2)))
    assert torch.equal(e2, lone(x, ti, C2))


# ------------------------------------------------------------------------------------------------
# the refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    PD.install_pair_double(monkeypatch, S, D)
    x = _x()
    dpm = _solver()
    P = "guidance over two conditions \\(cfg_pair\\): "
    with pytest.raises(NotImplementedError, match=P + "method='adaptive'"):
        dpm.sample(x, steps=6, order=2, method="adaptive")
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        dpm.sample_sde(x, steps=6, seed=1)
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        dpm.sample_sde_requests([x, x], steps=6, seeds=[1, 2])
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        dpm.sample_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        dpm.sample_unipc_requests([x, x], steps=6)
    with pytest.raises(NotImplementedError, match=P + "request_pool"):
        dpm.request_pool()
    with pytest.raises(NotImplementedError, match=P + "request_pool"):
        dpm.request_pool(slots=8)
    with pytest.raises(NotImplementedError, match=P + "correcting_x0_fn='dynamic_thresholding'"):
        _solver(correcting_x0_fn="dynamic_thresholding").sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "correcting_x0_fn='dynamic_thresholding'"):
        _solver(correcting_x0_fn="dynamic_thresholding").data_prediction_fn(x, torch.tensor([0.5]))
    with pytest.raises(NotImplementedError, match=P + "a callable correcting_x0_fn"):
        _solver(correcting_x0_fn=lambda x0, t: x0.clamp(-1, 1)).sample(x, steps=6, order=2)
    blend = D.MaskBlend(make_schedule("sd"), torch.ones(8, 8), x0=x, noise=x)
    with pytest.raises(NotImplementedError, match=P + "a MaskBlend corrector"):
        _solver(correcting_xt_fn=blend).sample(x, steps=6, order=2)
    # ... and none of them with the identity setting
    _solver(0.0, correcting_x0_fn="dynamic_thresholding").sample(x, steps=4, order=2)
    _solver(0.0).request_pool(slots=8)
    # a Python correcting_xt_fn, return_intermediate and denoise_to_zero are supported
    out, inter = _solver(correcting_xt_fn=lambda xt, t, step: xt * 0.999).sample(x, steps=4, order=2, denoise_to_zero=True,
                                                                               return_intermediate=True)
    assert torch.isfinite(out).all() and len(inter) == 6


# ------------------------------------------------------------------------------------------------
# the records
# ------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """the stage records that reach the launch entry points, as (flags, cfg_scale, cg_scale, guidance) in call order"""
    PD.install_pair_double(monkeypatch, S, D)
    seen = []
    raw, multi, stage = S._stage_launch_raw, S._stage_launch_multi_raw, S._launch_stage

    def rec(st):
        seen.append((int(st.flags), float(st.cfg_scale), float(st.cg_scale), int(st.guidance)))

    def raw_spy(st_ref, b_ref, stream):
        rec(st_ref._obj)
        b = b_ref._obj
        assert st_ref._obj.guidance != PAIR or (b.e1 and b.g and not b.x_out2 and not b.eps_stride)
        return raw(st_ref, b_ref, stream)

    def multi_spy(st_ref, bufs, n_req, stream):
        for r in range(int(n_req)):
            rec(st_ref._obj)
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
def test_binder_writes_s2_into_every_record(monkeypatch, algorithm_type, kw):
    seen = _spy(monkeypatch)
    x = _x(1)
    s2 = float(F32(1.5 - 3.0))
    ok = lambda rows: all(s == 3.0 and c == s2 and g == PAIR and not f & (L.F_THRESH | L.F_BLEND | L.F_NOISE) for f, s, c, g in rows)
    dpm = _solver(1.5, True, algorithm_type)
    out = dpm.sample(x, **kw)                                               # the prebuilt records (fast path)
    assert seen and ok(seen) and torch.isfinite(out).all()
    n_fast = len(seen)
    out_i, inter = dpm.sample(x, return_intermediate=True, **kw)            # the general loop binds the same records
    assert len(seen) == 2 * n_fast and ok(seen[n_fast:]) and torch.equal(out, out_i)
    del seen[:]
    outs = dpm.sample_requests([x, x + 1], **kw)                            # one multi-request call per stage
    assert len(seen) == 2 * n_fast and ok(seen) and torch.equal(outs[0], out)
    assert not torch.equal(out, _solver(None, False, algorithm_type).sample(x, **kw))


def test_cache_keys_change_with_the_setting(monkeypatch):
    seen = _spy(monkeypatch)
    x = _x(3)
    dpm = _solver(1.5)
    k0 = dpm._pair_key()
    a = dpm.sample(x, steps=4, order=2)
    n = len(seen)
    plans = len(dpm._plans)
    c2, s1, _ = dpm._wrapped.guidance_pair
    dpm._wrapped.guidance_pair = (c2, s1, 2.5)                               # another s2: other records, another plan entry
    b = dpm.sample(x, steps=4, order=2)
    assert dpm._pair_key() != k0 and len(dpm._plans) == plans + 1 and len(dpm._fast) == 2
    assert [c for f, s, c, g in seen[:n]] == [1.5] * n and [c for f, s, c, g in seen[n:]] == [2.5] * n
    dpm._wrapped.guidance_pair = (C2.clone(), s1, 2.5)                       # another condition tensor: another key
    assert dpm._pair_key() not in (k0, (id(c2), s1, 2.5))
    dpm._wrapped.guidance_pair = None                                        # off: classifier-free records
    c = dpm.sample(x, steps=4, order=2)
    assert all(g == CFG for f, s, cg, g in seen[2 * n:]) and dpm._pair_key() is None
    assert not torch.equal(a, b) and not torch.equal(b, c)


# ------------------------------------------------------------------------------------------------
# the planner
# ------------------------------------------------------------------------------------------------
def test_planner_accepts_guidance_3_and_writes_a_zero_s2():
    ns = make_schedule("sd")
    st = L.Stage()
    assert L.lib.dpm_coef_prologue(ns._h, 0.5, L.MODEL["v"], PAIR, 7.5, C.byref(st)) == 0
    ref = L.Stage()
    assert L.lib.dpm_coef_prologue(ns._h, 0.5, L.MODEL["v"], CFG, 7.5, C.byref(ref)) == 0
    assert st.guidance == PAIR and st.cfg_scale == ref.cfg_scale == 7.5 and st.cg_scale == 0.0 and ref.cg_scale != 0.0
    assert (st.alpha_e, st.sigma_e, st.t_input) == (ref.alpha_e, ref.sigma_e, ref.t_input)
    s64 = L.StageF64()
    assert L.lib.dpm_coef_prologue_f64(ns._h, 0.5, 0, L.MODEL["noise"], PAIR, 7.5, C.byref(st), C.byref(s64)) == 0
    assert st.guidance == PAIR and st.cg_scale == 0.0 and s64.cg_scale == 0.0 and s64.cfg_scale == 7.5
    assert L.lib.dpm_coef_prologue(ns._h, 0.5, 0, 4, 7.5, C.byref(st)) == L.ERR_ARG
    assert L.lib.dpm_last_error().decode() == "guidance out of range: 4"
    dpm = _solver(1.5)
    kw = dict(method="multistep", order=2, steps=6, skip_type="time_uniform", solver_type="dpmsolver", lower_order_final=True,
              denoise_to_zero=True, t_T=ns.T, t_0=1.0 / ns.total_N)
    plan, base = dpm._get_plan(**kw), _solver(None)._get_plan(**kw)
    assert len(plan.stages) == len(base.stages) == 7
    for a, b in zip(plan.stages, base.stages):
        assert a.guidance == PAIR and b.guidance == CFG and a.cfg_scale == b.cfg_scale == 3.0 and a.cg_scale == 0.0
        assert (a.form, a.flags, a.cx, a.c0, a.c1, a.t_eval) == (b.form, b.flags, b.cx, b.c0, b.c1, b.t_eval)
    d = L.PlanDesc()
    d.algorithm_type, d.order, d.steps, d.guidance, d.t_start, d.t_end = 1, 2, 6, 4, 1.0, 1e-3
    h = C.c_void_p()
    assert L.lib.dpm_plan_create(ns._h, C.byref(d), C.byref(h)) == L.ERR_ARG


# ------------------------------------------------------------------------------------------------
# the C side, before HIP
# ------------------------------------------------------------------------------------------------
def _record(form=L.FORM_TWO, flags=L.F_TO_X0 | L.F_STORE_M, guidance=PAIR, s1=7.5, s2=1.5, n=64, batch=2, dtype=L.DTYPE_F32):
    """a well-formed two-condition request on CPU pointers (never read: the calls below end before any launch)"""
    arena = np.zeros(10 * n * 8 + 64, dtype=np.uint8)
    base = (arena.ctypes.data + 63) // 64 * 64
    st, b = L.Stage(), L.Buffers()
    st.form, st.flags, st.guidance, st.model_type = form, flags, guidance, L.MODEL["noise"]
    st.alpha_e, st.sigma_e, st.cfg_scale, st.cg_scale = 0.8, 0.6, s1, s2
    st.cx, st.c0, st.c1 = 0.9, -0.1, 0.05
    st.h1_slot = st.h2_slot = st.m_slot = -1
    p = [base + k * n * 8 for k in range(10)]
    b.x, b.e0, b.e1, b.g, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]
    b.n, b.batch, b.state_dtype, b.eps_dtype = n, batch, dtype, dtype
    return st, b, arena


TX = L.F_TO_X0
SPLIT = "stage_launch: DPM_GUIDE_CFG2 with thresholding, mask blend, noise or a split stage (flags %d)"
TEXTS = [   # every refusal, in the order dpm_stage_launch asks: return code and the whole message
    (dict(flags=TX | L.F_CFG_RESCALE), L.ERR_ARG, "stage_launch: DPM_F_CFG_RESCALE is valid under classifier-free guidance only (guidance 3)"),
    (dict(flags=TX | L.F_CFG_APG), L.ERR_ARG, "stage_launch: DPM_F_CFG_APG is valid under classifier-free guidance only (guidance 3)"),
    (dict(flags=TX | L.F_CFG_ZSTAR), L.ERR_ARG, "stage_launch: DPM_F_CFG_ZSTAR is valid under classifier-free guidance only (guidance 3)"),
    (dict(s1=float("nan")), L.ERR_ARG,
     "stage_launch: DPM_GUIDE_CFG2 with s1=nan (dpm_stage.cfg_scale), s2=1.5 (dpm_stage.cg_scale): both must be finite"),
    (dict(s2=float("inf")), L.ERR_ARG,
     "stage_launch: DPM_GUIDE_CFG2 with s1=7.5 (dpm_stage.cfg_scale), s2=inf (dpm_stage.cg_scale): both must be finite"),
    (dict(flags=TX | L.F_THRESH), L.ERR_UNSUPPORTED, SPLIT % (TX | L.F_THRESH)),
    (dict(flags=TX | L.F_BLEND), L.ERR_UNSUPPORTED, SPLIT % (TX | L.F_BLEND)),
    (dict(flags=TX | L.F_NOISE), L.ERR_UNSUPPORTED, SPLIT % (TX | L.F_NOISE)),
    (dict(flags=TX | L.F_USER_X0), L.ERR_UNSUPPORTED, SPLIT % (TX | L.F_USER_X0)),
    (dict(form=L.FORM_UNIPC), L.ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 on a DPM_FORM_UNIPC stage"),
    (dict(form=6), L.ERR_ARG, "unknown update form 6"),
    (dict(form=-1), L.ERR_ARG, "unknown update form -1"),
    (dict(x_out2=True), L.ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with x_out2 (the kernel has no second store)"),
    (dict(dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with a double state (no double kernel)"),
    (dict(stride=40), L.ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with eps_stride=40 (a channel slice of a wider output)"),
    (dict(null="e1"), L.ERR_ARG, "stage_launch: DPM_GUIDE_CFG2 needs e1 and g"),
    (dict(null="g"), L.ERR_ARG, "stage_launch: DPM_GUIDE_CFG2 needs e1 and g"),
    # ... and which of two speaks first
    (dict(flags=TX | L.F_CFG_ZSTAR | L.F_NOISE, s2=float("nan")), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_ZSTAR is valid under classifier-free guidance only (guidance 3)"),
    (dict(s2=float("-inf"), flags=TX | L.F_NOISE, dtype=L.DTYPE_F64), L.ERR_ARG,
     "stage_launch: DPM_GUIDE_CFG2 with s1=7.5 (dpm_stage.cfg_scale), s2=-inf (dpm_stage.cg_scale): both must be finite"),
    (dict(flags=TX | L.F_NOISE, form=6, dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED, SPLIT % (TX | L.F_NOISE)),
    (dict(form=L.FORM_UNIPC, x_out2=True, dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 on a DPM_FORM_UNIPC stage"),
    (dict(x_out2=True, dtype=L.DTYPE_F64, stride=40, null="g"), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_GUIDE_CFG2 with x_out2 (the kernel has no second store)"),
    (dict(dtype=L.DTYPE_F64, stride=40, null="g"), L.ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with a double state (no double kernel)"),
]


@pytest.mark.parametrize("kw,code,text", TEXTS, ids=[str(i) for i in range(len(TEXTS))])
def test_every_refusal_has_its_code_its_text_and_its_turn(kw, code, text):
    kw = dict(kw)
    stride, null, xo2 = kw.pop("stride", 0), kw.pop("null", None), kw.pop("x_out2", False)
    st, b, arena = _record(**kw)
    b.eps_stride = stride
    if null:
        setattr(b, null, None)
    if xo2:
        b.x_out2 = b.m_out + 8 * b.n
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


def test_device_resident_coefficients_are_refused_in_so_many_words():
    """dpm_adaptive_stage_launch hands the stage the ADDRESS of a coefficient record in the handle's device block and refuses
    the guidance before anything reads it: zeroed host memory stands in for the handle (no device to create one on)"""
    st, b, arena = _record()
    handle = np.zeros(1 << 16, dtype=np.uint8)
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    assert L.lib.dpm_last_error().decode() == "stage_launch: DPM_GUIDE_CFG2 with device-resident coefficients"
    assert not arena.any() and not handle.any()
    st.cg_scale = float("nan")                              # the record's own errors come first
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_ARG


def test_an_empty_batch_is_ok_and_its_record_is_still_checked():
    st, b, _ = _record(n=0, batch=1)
    b.e1 = b.g = None                                       # (nothing would be read)
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == 0
    st.cg_scale = float("nan")
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_ARG


def test_eps_stride_equal_to_the_sample_is_dense():
    st, b, _ = _record(form=6)                              # passes the stride rule ... and has failed an earlier one: the form
    b.eps_stride = b.n // b.batch
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_ARG
    st.form, b.eps_stride, b.x_out2 = L.FORM_TWO, b.n // b.batch, b.m_out + 8 * b.n
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    assert "x_out2" in L.lib.dpm_last_error().decode()


def test_table_fill_gives_a_two_condition_request_no_row():
    """20 fusable TWO requests, classifier-free: one run of 20 rows.  Make request 7 a two-condition one and the run has 19 -- in
    call order, without it -- whatever table flags the call carries; DPM_TABLE_FILL launches nothing and never calls HIP."""
    HDR, ROW = L.TABLE_HEADER_BYTES, L.TABLE_ROW_BYTES
    R, N = 20, 2048

    def call(pair, extra=0):
        st, bs = (L.Stage * R)(), (L.Buffers * R)()
        arena = np.zeros(R * 9 * N * 2 + 64, dtype=np.uint8)
        base = (arena.ctypes.data + 63) // 64 * 64
        for r in range(R):
            s, b = st[r], bs[r]
            s.form, s.flags, s.guidance = L.FORM_TWO, L.F_TO_X0 | L.F_STORE_M, CFG
            s.alpha_e, s.sigma_e, s.cfg_scale, s.cg_scale = 0.8, 0.6, 7.5, 0.7
            p = [base + (r * 9 + k) * N * 2 for k in range(9)]
            b.x, b.e0, b.e1, b.h1, b.x_out, b.m_out, b.x_out2 = p[0], p[1], p[2], p[3], p[5], p[6], p[7]
            if r in pair:
                s.guidance, b.g, b.x_out2 = PAIR, p[8], None
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
    for extra in (0, L.TABLE_RESCALE | L.TABLE_APG | L.TABLE_ZSTAR | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_NOISE):
        body, rows, xs, _a = call({7}, extra)
        assert [int(v) for v in body[:16].view(np.uint32)] == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
        assert rows(R - 1)[:, 0].tolist() == [x for r, x in enumerate(xs) if r != 7]
        assert bool((body[HDR + (R - 1) * ROW:HDR + R * ROW] == 0xAB).all())


# ------------------------------------------------------------------------------------------------
# the double, the torch statement and sample() against float64
# ------------------------------------------------------------------------------------------------
def _blend64(w, x, t, s1, s2, c2):
    """the contract in torch float64 on a float64 x: conversions per output, then the three-branch blend"""
    ns = w.noise_schedule
    ti = w.get_model_input_time(t)
    outs = [w.model(x, ti, c.to(x.dtype)) for c in (w.condition, w.unconditional_condition, c2)]
    al, sg = (v.reshape(-1, 1, 1, 1).double() for v in (ns.marginal_alpha(t), ns.marginal_std(t)))

    def to_noise(o):
        return {"noise": lambda: o, "x_start": lambda: (x - al * o) / sg, "v": lambda: al * o + sg * x, "score": lambda: -sg * o}[w.model_type]()
    n0, n1, n2 = (to_noise(o) for o in outs)
    return n1 + s1 * (n0 - n1) + s2 * (n2 - n1)


@pytest.mark.parametrize("ed", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("model_type", ["noise", "x_start", "v", "score"])
def test_double_restates_the_contract(ed, model_type):
    """the numpy double against a float64 evaluation of the formula (1e-6 of the scale: a handful of fp32 roundings -- nothing
    is rounded to the network's dtype after the loads), and its two identities bit for bit"""
    rng = np.random.default_rng(11)
    n = 4100
    st, _, _ = _record(form=L.FORM_LIN1, flags=0)
    st.model_type = L.MODEL[model_type]
    rnd = KD.half_rounder(ed) or (lambda a: a)
    e0, e1, e2 = (rnd(rng.standard_normal(n).astype(F32)) for _ in range(3))
    x = rng.standard_normal(n).astype(F32)
    out, mn = PD.stage(st, x, x, e0, e1, e2, None, None)
    c = KD._Coef(st)
    n0, n1, n2 = (KD.to_noise(o.astype(np.float64), x.astype(np.float64), KD._Coef(st, np.float64)) for o in (e0, e1, e2))
    want = n1 + 7.5 * (n0 - n1) + 1.5 * (n2 - n1)
    assert float(np.abs(mn - want).max() / np.abs(want).max()) <= 1e-6
    assert np.array_equal(out, (F32(0.9) * x - F32(-0.1) * mn).astype(F32))
    # g == e1: d2 is an exact zero, s2 * 0 = 0, (a + 0) = a -- the fp32 classifier-free blend
    _, mn_same = PD.stage(st, x, x, e0, e1, e1, None, None)
    cf = (n1_32 := np.asarray(KD.to_noise(e1, x, c), dtype=F32)) + (c.cfg_scale * (np.asarray(KD.to_noise(e0, x, c), dtype=F32) - n1_32).astype(F32)).astype(F32)
    assert np.array_equal(mn_same, cf.astype(F32))
    st.cg_scale = 0.0                                        # s2 == 0: the same
    assert np.array_equal(PD.stage(st, x, x, e0, e1, e2, None, None)[1], cf.astype(F32))


@pytest.mark.parametrize("model_type", ["noise", "v"])
def test_call_is_the_torch_statement_and_nested_is_instructpix2pix_written_out(monkeypatch, model_type):
    PD.install_pair_double(monkeypatch, S, D)
    fn, ns = _wrapper(model_type=model_type, scale=7.5)                      # s_T = 7.5 (text), s_I = 1.5 (image)
    w = D.cfg_pair(fn, C2, 1.5, nested=True)                                 # condition = image + text, condition2 = image alone
    x = _x(5)
    t = torch.full((2,), 0.6)
    got = w(x, t)
    assert got.dtype is torch.float32
    xd = x.double()
    ti = w.get_model_input_time(t)
    al, sg = (v.reshape(-1, 1, 1, 1).double() for v in (ns.marginal_alpha(t), ns.marginal_std(t)))
    conv = (lambda o: o) if model_type == "noise" else (lambda o: al * o + sg * xd)
    e_u, e_i, e_it = (conv(w.model(xd, ti, c.double())) for c in (w.unconditional_condition, C2, w.condition))
    want = e_u + 1.5 * (e_i - e_u) + 7.5 * (e_it - e_i)                      # InstructPix2Pix, eq. 3
    assert float((got.double() - want).abs().max() / want.abs().max()) <= 1e-6
    assert float((_blend64(w, xd, t, 7.5, 1.5 - 7.5, C2) - want).abs().max() / want.abs().max()) <= 1e-12
    # ... and a one-stage DENOISE launch of the double gives __call__'s bits (fp32 outputs)
    dpm = D.DPM_Solver(w, ns, algorithm_type="dpmsolver")
    assert torch.equal(dpm.noise_prediction_fn(x, torch.tensor([0.6])), got)


@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("algorithm_type,kw", [("dpmsolver++", dict(steps=6, order=2)), ("dpmsolver", dict(steps=6, order=3)),
                                               ("dpmsolver++", dict(steps=6, order=3, method="singlestep")),
                                               ("dpmsolver++", dict(steps=5, order=2, denoise_to_zero=True))],
                         ids=["2M++", "3M", "3S++", "2M++dz"])
def test_sample_on_the_double_against_a_torch_float64_statement(monkeypatch, model_type, algorithm_type, kw):
    """sample() under cfg_pair, fp32 state, kernels replaced by the numpy double -- against the SAME sampler in float64 on a
    model callable that blends the three branches in torch float64 (what a caller had to write before cfg_pair existed)"""
    PD.install_pair_double(monkeypatch, S, D)
    x = _x(7)
    dpm = _solver(1.5, True, algorithm_type, model_type=model_type)
    got = dpm.sample(x, **kw)
    w, ns = dpm._wrapped, dpm.noise_schedule
    ref = D.DPM_Solver(lambda xx, tt: _blend64(w, xx, tt, 3.0, 1.5 - 3.0, C2), ns, algorithm_type=algorithm_type)
    want = ref.sample(x.double(), **kw)
    assert want.dtype is torch.float64 and got.dtype is torch.float32
    assert float((got.double() - want).abs().max() / want.abs().max()) <= 1e-5
    # a double state: the three outputs are blended in torch, in double, and the stage is unguided
    got64 = dpm.sample(x.double(), **kw)
    assert got64.dtype is torch.float64 and float((got64 - want).abs().max() / want.abs().max()) <= 1e-12
    outs64 = dpm.sample_requests([x.double(), x.double() + 1], **kw)
    assert torch.equal(outs64[0], got64)


# ------------------------------------------------------------------------------------------------
# a channel slice of a wider output (a learned-variance network's out[:, :C]): three dense outputs on every path
# ------------------------------------------------------------------------------------------------
class WideNet(Net):
    """answers [3B, 2C, H, W]; the caller keeps the first C channels -- samples dense, a wide output's stride apart"""

    def __call__(self, x, t, c):
        y = super().__call__(x, t, c)
        return torch.cat([y, 0.5 * y - 1.0], dim=1)[:, :y.shape[1]]


def test_bind_outputs_takes_no_slice_for_a_two_condition_record():
    from dpm_solver_amd.launch_list import _bind_outputs
    wide = torch.randn(6, 6, 8, 8, generator=torch.Generator().manual_seed(5))
    e1, e0, e2 = wide[:, :3].chunk(3)
    assert not e0.is_contiguous() and e0.stride(0) == 6 * 64
    b = L.Buffers()
    keep = _bind_outputs(b, e0, e1, e2, torch.float32, e0.shape, None, True)
    assert b.eps_stride == 0 and all(k.is_contiguous() for k in keep)
    assert (b.e0, b.e1, b.g) == tuple(k.data_ptr() for k in keep)
    assert all(torch.equal(k, e) for k, e in zip(keep, (e0, e1, e2)))
    # ... where the two-branch records read the slice in place, as before
    b = L.Buffers()
    keep = _bind_outputs(b, e0, e1, None, torch.float32, e0.shape)
    assert b.eps_stride == 6 * 64 and b.e0 == e0.data_ptr() and b.e1 == e1.data_ptr() and keep[0] is e0
    # dense outputs are bound as they are
    d0, d1, d2 = (t.contiguous() for t in (e0, e1, e2))
    b = L.Buffers()
    keep = _bind_outputs(b, d0, d1, d2, torch.float32, d0.shape, None, True)
    assert b.eps_stride == 0 and keep[0] is d0 and keep[1] is d1 and keep[2] is d2


@pytest.mark.parametrize("kw", [dict(steps=6, order=2), dict(steps=6, order=3, method="singlestep")], ids=["2M", "3S"])
def test_a_sliced_network_runs_on_every_path_and_equals_the_dense_one(monkeypatch, kw):
    """sample() (the prebuilt records), return_intermediate (the general loop), sample_requests (the multi-request call) and a
    double state under a [3B, 2C, H, W] network sliced to C channels, on the double: the dense network's bits.  The spy refuses
    a two-condition record with an eps_stride, and the double reads dense operands only."""
    seen = _spy(monkeypatch)
    x = _x(9)
    want = _solver(1.5, True).sample(x, **kw)
    n = len(seen)
    dpm = _solver(1.5, True, net=WideNet())
    assert torch.equal(dpm.sample(x, **kw), want) and len(seen) == 2 * n
    out_i, inter = dpm.sample(x, return_intermediate=True, **kw)
    assert torch.equal(out_i, want) and len(seen) == 3 * n
    outs = dpm.sample_requests([x, x + 1], **kw)
    assert torch.equal(outs[0], want) and torch.equal(outs[1], _solver(1.5, True).sample(x + 1, **kw))
    assert all(g == PAIR for f, s, c, g in seen)
    assert torch.equal(dpm.sample(x.double(), **kw), _solver(1.5, True).sample(x.double(), **kw))


def test_the_tripled_time_is_built_once_per_plan_and_batch(monkeypatch):
    """the loops hand raw_outputs the plan's cached (3B,) time vector of the stage -- no torch.cat of the time per evaluation"""
    PD.install_pair_double(monkeypatch, S, D)
    times = []

    class TNet(Net):
        def __call__(self, x, t, c):
            times.append(t)
            return super().__call__(x, t, c)
    dpm = _solver(1.5, net=TNet())
    x = _x(2)
    a = dpm.sample(x, steps=4, order=2)
    first = list(times)
    del times[:]
    b = dpm.sample(x, steps=4, order=2)
    assert torch.equal(a, b) and len(first) == len(times) == 4
    assert all(t.shape == (6,) and t.is_contiguous() and float(t.min()) == float(t.max()) for t in first)
    assert all(s.data_ptr() == t.data_ptr() for s, t in zip(first, times))       # the same vectors, call after call
    del times[:]
    dpm.sample(x, steps=4, order=2, return_intermediate=True)
    assert all(s.data_ptr() == t.data_ptr() for s, t in zip(first, times))       # ... and in the general loop
    # classifier-free guidance keeps its doubled ones
    del times[:]
    _solver(None, net=TNet()).sample(x, steps=4, order=2)
    assert all(t.shape == (4,) for t in times)
