"""Guidance rescale (dpm_solver_amd.cfg_rescale, DPM_F_CFG_RESCALE; C ABI version 212) without a GPU: the helper, every
refusal, the stage records the binder builds (the kernels replaced by the numpy doubles), the argument errors dpm_stage_launch
decides before it touches HIP, a DPM_TABLE_FILL call, and WrappedModel.__call__ against the diffusers expression."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import rescale_double as RD
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule

CFG = L.GUIDE["classifier-free"]


def _net(x, t, c):
    return torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]) + 0.05 * x


def _wrapper(model_type="noise", scale=3.0, uncond=True, ns=None):
    ns = ns or make_schedule("sd")
    c = torch.ones(2)
    return D.model_wrapper(_net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=scale, condition=c,
                           unconditional_condition=c * 0 if uncond else None), ns


def _solver(phi=0.7, algorithm_type="dpmsolver++", **kw):
    wkw = {k: kw.pop(k) for k in ("model_type", "scale", "uncond") if k in kw}
    fn, ns = _wrapper(**wkw)
    return D.DPM_Solver(D.cfg_rescale(fn, phi) if phi is not None else fn, ns, algorithm_type=algorithm_type, **kw)


# ------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------
def test_abi_212_flag_and_binding():
    assert L.lib.dpm_version() >= 212 and L.F_CFG_RESCALE == 1024
    assert C.sizeof(L.Stage) == L.lib.dpm_sizeof(0) and C.sizeof(L.Buffers) == L.lib.dpm_sizeof(1)


def test_helper_returns_a_copy_with_phi_set():
    fn, _ = _wrapper()
    assert fn.guidance_rescale == 0.0 and fn.rescale_phi == 0.0
    out = D.cfg_rescale(fn, 0.7)
    assert isinstance(out, D.WrappedModel) and out is not fn and out.guidance_rescale == 0.7 and out.rescale_phi == 0.7
    assert fn.guidance_rescale == 0.0                                       # the original is untouched
    assert out.model is fn.model and out.condition is fn.condition and out.guidance_scale == fn.guidance_scale
    assert D.cfg_rescale(fn, 1).guidance_rescale == 1.0 and D.cfg_rescale(fn, 0).rescale_phi == 0.0
    assert D.cfg_rescale(fn, np.float32(0.5)).guidance_rescale == 0.5
    # no classifier-free blend -> nothing to rescale: the flag is never asked for
    assert D.cfg_rescale(_wrapper(scale=1.0)[0], 0.7).rescale_phi == 0.0
    assert D.cfg_rescale(_wrapper(uncond=False)[0], 0.7).rescale_phi == 0.0


@pytest.mark.parametrize("phi", [-0.1, 1.5, float("nan"), "0.7", None, True, 1j])
def test_helper_refuses_a_phi_outside_0_1(phi):
    with pytest.raises(ValueError, match="phi must be a real number in \\[0, 1\\]"):
        D.cfg_rescale(_wrapper()[0], phi)


def test_helper_refuses_anything_but_a_classifier_free_wrapper():
    ns = make_schedule("sd")
    for bad in (lambda x, t: x, D.model_wrapper(lambda x, t: x, ns), D.model_wrapper(
            lambda x, t: x, ns, guidance_type="classifier", classifier_fn=lambda *a: 0, condition=torch.ones(1))):
        with pytest.raises(ValueError, match="guidance_type='classifier-free'"):
            D.cfg_rescale(bad, 0.5)


# ------------------------------------------------------------------------------------------------
# the refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    RD.install_rescale_double(monkeypatch, S, D)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(0))
    dpm = _solver()
    with pytest.raises(NotImplementedError, match="guidance rescale.*method='adaptive'"):
        dpm.sample(x, steps=6, order=2, method="adaptive")
    with pytest.raises(NotImplementedError, match="guidance rescale.*method='adaptive'"):
        dpm.dpm_solver_adaptive(x, 2, 1.0, 1e-3)
    with pytest.raises(NotImplementedError, match="guidance rescale.*sample_sde"):
        dpm.sample_sde(x, steps=6, seed=1)
    with pytest.raises(NotImplementedError, match="guidance rescale.*sample_sde"):
        dpm.sample_sde_requests([x, x], steps=6, seeds=[1, 2])
    with pytest.raises(NotImplementedError, match="guidance rescale.*sample_unipc"):
        dpm.sample_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match="guidance rescale.*sample_unipc"):
        dpm.sample_unipc_requests([x, x], steps=6)
    with pytest.raises(NotImplementedError, match="guidance rescale.*slab pool"):
        dpm.request_pool(slots=8)
    pool = dpm.request_pool()
    with pytest.raises(NotImplementedError, match="guidance rescale.*sample_sde"):
        pool.submit(x, steps=6, sde=True, seed=3)
    with pytest.raises(NotImplementedError, match="guidance rescale.*sample_unipc"):
        pool.submit_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match="guidance rescale.*dynamic_thresholding"):
        _solver(correcting_x0_fn="dynamic_thresholding").sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match="guidance rescale.*dynamic_thresholding"):
        _solver(correcting_x0_fn="dynamic_thresholding").data_prediction_fn(x, torch.tensor([0.5]))
    blend = D.MaskBlend(make_schedule("sd"), torch.ones(8, 8), x0=x, noise=x)
    with pytest.raises(NotImplementedError, match="guidance rescale.*MaskBlend"):
        _solver(correcting_xt_fn=blend).sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match="guidance rescale.*double-precision"):
        dpm.sample(x.double(), steps=6, order=2)
    with pytest.raises(NotImplementedError, match="guidance rescale.*double-precision"):
        dpm.sample_requests([x.double(), x.double()], steps=6, order=2)
    # ... and only where a stage is thresholded: the noise prediction of a thresholding solver involves no thresholding
    assert torch.isfinite(_solver(correcting_x0_fn="dynamic_thresholding").noise_prediction_fn(x, torch.tensor([0.5]))).all()
    # phi = 0 refuses nothing
    _solver(0.0, correcting_x0_fn="dynamic_thresholding").sample(x, steps=4, order=2)


# ------------------------------------------------------------------------------------------------
# the records
# ------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """the stage records that reach the launch entry points, as (flags, cg_scale, guidance) in call order"""
    RD.install_rescale_double(monkeypatch, S, D)
    seen = []
    raw, multi, stage = S._stage_launch_raw, S._stage_launch_multi_raw, S._launch_stage

    def rec(st):
        seen.append((int(st.flags), float(st.cg_scale), int(st.guidance)))

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


RUNS = [dict(steps=6, order=2), dict(steps=6, order=3), dict(steps=6, order=3, method="singlestep"),
        dict(steps=6, order=2, method="singlestep_fixed", solver_type="taylor"), dict(steps=5, order=1, denoise_to_zero=True)]


@pytest.mark.parametrize("algorithm_type", ["dpmsolver", "dpmsolver++"])
@pytest.mark.parametrize("kw", RUNS, ids=lambda k: "%s%d" % (k.get("method", "multistep"), k["order"]))
def test_flag_and_phi_reach_every_record(monkeypatch, algorithm_type, kw):
    seen = _spy(monkeypatch)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    phi = float(np.float32(0.7))
    dpm = _solver(0.7, algorithm_type)
    out = dpm.sample(x, **kw)                                               # the prebuilt records (fast path)
    assert seen and all(f & L.F_CFG_RESCALE and c == phi and g == CFG for f, c, g in seen)
    n_fast = len(seen)
    out_i, inter = dpm.sample(x, return_intermediate=True, **kw)            # the general loop binds the same records
    assert len(seen) == 2 * n_fast and all(f & L.F_CFG_RESCALE and c == phi for f, c, g in seen[n_fast:])
    assert torch.equal(out, out_i) and torch.isfinite(out).all()
    del seen[:]
    outs = dpm.sample_requests([x, x + 1], **kw)                            # one multi-request call per stage
    assert len(seen) == 2 * n_fast and all(f & L.F_CFG_RESCALE and c == phi for f, c, g in seen)     # (seen per request)
    assert torch.equal(outs[0], out)
    del seen[:]
    pool = dpm.request_pool()                                               # a RequestPool without slots accepts the solver
    h = [pool.submit(x, **kw), pool.submit(x + 1, **kw)]
    done = {}
    while pool:
        done.update(pool.step())
    assert len(seen) == 2 * n_fast and all(f & L.F_CFG_RESCALE and c == phi for f, c, g in seen)
    assert torch.equal(done[h[0]], out) and torch.equal(done[h[1]], outs[1])


@pytest.mark.parametrize("how", ["phi0", "scale1", "no_uncond", "no_helper"])
def test_flag_is_absent_and_every_bit_is_todays(monkeypatch, how):
    seen = _spy(monkeypatch)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2))
    wkw = {"scale1": dict(scale=1.0), "no_uncond": dict(uncond=False)}.get(how, {})
    plain = _solver(None, **wkw).sample(x, steps=6, order=2)
    cgs = [c for f, c, g in seen]
    del seen[:]
    got = _solver(None if how == "no_helper" else (0.0 if how == "phi0" else 0.7), **wkw).sample(x, steps=6, order=2)
    assert seen and not any(f & L.F_CFG_RESCALE for f, c, g in seen)
    assert [c for f, c, g in seen] == cgs                                   # cg_scale stays the planner's
    assert torch.equal(got, plain)


def test_changing_phi_on_the_wrapper_misses_the_cached_records(monkeypatch):
    seen = _spy(monkeypatch)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(3))
    dpm = _solver(0.7)
    a = dpm.sample(x, steps=4, order=2)
    dpm._wrapped.guidance_rescale = 0.25
    b = dpm.sample(x, steps=4, order=2)
    assert {c for f, c, g in seen[len(seen) // 2:]} == {0.25} and not torch.equal(a, b)


def test_split_stage_around_a_callable_x0_corrector_keeps_the_rescale(monkeypatch):
    seen = _spy(monkeypatch)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(4))
    _solver(0.7, correcting_x0_fn=lambda x0, t: x0.clamp(-1, 1)).sample(x, steps=4, order=2)
    pro = [s for s in seen if s[2] == CFG]                                  # the prologue halves carry the blend
    assert pro and all(f & L.F_CFG_RESCALE for f, c, g in pro)
    assert not any(f & L.F_CFG_RESCALE for f, c, g in seen if g != CFG)     # the update halves have no network output


# ------------------------------------------------------------------------------------------------
# the C side, before HIP
# ------------------------------------------------------------------------------------------------
def _record(form=L.FORM_TWO, flags=L.F_TO_X0 | L.F_STORE_M | L.F_CFG_RESCALE, guidance=CFG, phi=0.7, n=64, batch=2,
            dtype=L.DTYPE_F32):
    """a well-formed flagged request on CPU pointers (never read: the calls below end before any launch)"""
    arena = np.zeros(10 * n * 8 + 64, dtype=np.uint8)
    base = (arena.ctypes.data + 63) // 64 * 64
    st, b = L.Stage(), L.Buffers()
    st.form, st.flags, st.guidance, st.model_type = form, flags, guidance, L.MODEL["noise"]
    st.alpha_e, st.sigma_e, st.cfg_scale, st.cg_scale = 0.8, 0.6, 7.5, phi
    st.cx, st.c0, st.c1 = 0.9, -0.1, 0.05
    st.h1_slot = st.h2_slot = st.m_slot = -1
    p = [base + k * n * 8 for k in range(9)]
    b.x, b.e0, b.e1, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[2], p[3], p[4], p[5], p[6]
    b.n, b.batch, b.state_dtype, b.eps_dtype = n, batch, dtype, dtype
    return st, b, arena


BAD = [
    (dict(guidance=L.GUIDE["uncond"]), L.ERR_ARG, "classifier-free guidance only"),
    (dict(guidance=L.GUIDE["classifier"]), L.ERR_ARG, "classifier-free guidance only"),
    (dict(n=3, batch=3), L.ERR_ARG, "at least 2 elements"),
    (dict(phi=1.5), L.ERR_ARG, "not in (0, 1]"),
    (dict(phi=0.0), L.ERR_ARG, "not in (0, 1]"),
    (dict(phi=-0.5), L.ERR_ARG, "not in (0, 1]"),
    (dict(phi=float("nan")), L.ERR_ARG, "not in (0, 1]"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE | L.F_THRESH), L.ERR_UNSUPPORTED, "thresholding, mask blend or noise"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE | L.F_BLEND), L.ERR_UNSUPPORTED, "thresholding, mask blend or noise"),
    (dict(flags=L.F_TO_X0 | L.F_CFG_RESCALE | L.F_NOISE), L.ERR_UNSUPPORTED, "thresholding, mask blend or noise"),
    (dict(form=L.FORM_UNIPC), L.ERR_UNSUPPORTED, "DPM_FORM_UNIPC"),
    (dict(form=6), L.ERR_ARG, "unknown update form 6"),
    (dict(form=-1), L.ERR_ARG, "unknown update form -1"),
    (dict(dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, "double state"),
    (dict(stride=40), L.ERR_UNSUPPORTED, "eps_stride"),
]


@pytest.mark.parametrize("kw,code,text", BAD, ids=[t[2][:12] + str(i) for i, t in enumerate(BAD)])
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
    assert not arena.any() and not arena2.any()
    with pytest.raises(ValueError if code == L.ERR_ARG else NotImplementedError):
        L.check(code)


RS = L.F_TO_X0 | L.F_CFG_RESCALE
TEXTS = [   # every refusal of the flag, in the order dpm_stage_launch asks: return code and the whole message
    (dict(guidance=L.GUIDE["classifier"]), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_RESCALE is valid under classifier-free guidance only (guidance 2)"),
    (dict(n=3, batch=3), L.ERR_ARG, "stage_launch: DPM_F_CFG_RESCALE needs samples of at least 2 elements (got 1)"),
    (dict(phi=1.5), L.ERR_ARG, "stage_launch: DPM_F_CFG_RESCALE with phi=1.5 (dpm_stage.cg_scale), which is not in (0, 1]"),
    (dict(flags=RS | L.F_THRESH), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE with thresholding, mask blend or noise (flags 1033)"),
    (dict(form=L.FORM_UNIPC), L.ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG_RESCALE on a DPM_FORM_UNIPC stage"),
    (dict(form=6), L.ERR_ARG, "unknown update form 6"),
    (dict(dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG_RESCALE with a double state (no double rescale kernel)"),
    (dict(stride=40), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE with eps_stride=40 (a channel slice of a wider output)"),
    # ... and which of two speaks first: each row fails the check of its own line and every later one it can
    (dict(guidance=0, n=3, batch=3, phi=0.0, flags=RS | L.F_NOISE, form=6, dtype=L.DTYPE_F64, stride=40), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_RESCALE is valid under classifier-free guidance only (guidance 0)"),
    (dict(n=3, batch=3, phi=0.0, flags=RS | L.F_NOISE, form=6, dtype=L.DTYPE_F64, stride=40), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_RESCALE needs samples of at least 2 elements (got 1)"),
    (dict(phi=0.0, flags=RS | L.F_NOISE, form=6, dtype=L.DTYPE_F64, stride=40), L.ERR_ARG,
     "stage_launch: DPM_F_CFG_RESCALE with phi=0 (dpm_stage.cg_scale), which is not in (0, 1]"),
    (dict(flags=RS | L.F_NOISE, form=6, dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE with thresholding, mask blend or noise (flags 1089)"),
    (dict(flags=RS | L.F_BLEND, form=L.FORM_UNIPC, dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE with thresholding, mask blend or noise (flags 1057)"),
    (dict(form=L.FORM_UNIPC, dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE on a DPM_FORM_UNIPC stage"),
    (dict(form=-1, dtype=L.DTYPE_F64, stride=40), L.ERR_ARG, "unknown update form -1"),
    (dict(dtype=L.DTYPE_F64, stride=40), L.ERR_UNSUPPORTED,
     "stage_launch: DPM_F_CFG_RESCALE with a double state (no double rescale kernel)"),
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
    assert L.lib.dpm_last_error().decode() == "stage_launch: DPM_F_CFG_RESCALE with device-resident coefficients"
    assert not arena.any() and not handle.any()
    st.cg_scale = 1.5                                   # the record's own errors come first
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_ARG
    assert "not in (0, 1]" in L.lib.dpm_last_error().decode()


def test_an_empty_batch_is_ok_and_its_record_is_still_checked():
    """n == 0 launches nothing and returns DPM_OK, as for every stage (the sample-size rule has no sample to apply to);
    the record's own errors are reported all the same"""
    st, b, _ = _record(n=0, batch=1)
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == 0
    st.cg_scale = 1.5
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_ARG


def test_eps_stride_equal_to_the_sample_is_dense():
    st, b, _ = _record(phi=float("nan"))            # passes the stride rule and fails the next one it meets: phi
    b.eps_stride = b.n // b.batch
    st.cg_scale = 0.5
    st.form = L.FORM_UNIPC
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    assert "DPM_FORM_UNIPC" in L.lib.dpm_last_error().decode()


def test_table_fill_gives_a_flagged_request_no_row():
    """20 fusable TWO requests, classifier-free: one run of 20 rows.  Flag request 7 and the run has 19 -- in call order,
    without it -- and nothing else of the table changes shape; DPM_TABLE_FILL launches nothing and never calls HIP."""
    HDR, ROW = L.TABLE_HEADER_BYTES, L.TABLE_ROW_BYTES
    R, N = 20, 2048

    def call(flagged):
        st, bs = (L.Stage * R)(), (L.Buffers * R)()
        arena = np.zeros(R * 9 * N * 2 + 64, dtype=np.uint8)
        base = (arena.ctypes.data + 63) // 64 * 64
        for r in range(R):
            s, b = st[r], bs[r]
            s.form, s.flags, s.guidance = L.FORM_TWO, L.F_TO_X0 | L.F_STORE_M, CFG
            s.alpha_e, s.sigma_e, s.cfg_scale, s.cg_scale = 0.8, 0.6, 7.5, 4.5
            if r in flagged:
                s.flags |= L.F_CFG_RESCALE
                s.cg_scale = 0.7
            p = [base + (r * 9 + k) * N * 2 for k in range(9)]
            b.x, b.e0, b.e1, b.h1, b.x_out, b.m_out, b.x_out2 = p[0], p[1], p[2], p[3], p[5], p[6], p[7]
            b.n, b.batch, b.state_dtype, b.eps_dtype = N, 2, L.DTYPE_F16, L.DTYPE_F16
        opts = L.LaunchOpts()
        opts.per_request_stages, opts.table_mode = 1, L.TABLE_FILL
        bs[0].opts = C.pointer(opts)
        table = np.full(HDR + R * ROW + 16, 0xAB, dtype=np.uint8)
        off = (-table.ctypes.data) % 16
        bs[0].workspace = table.ctypes.data + off
        assert L.lib.dpm_stage_launch_multi(st, bs, R, None) == 0, L.lib.dpm_last_error()
        body = table[off:off + HDR + R * ROW]
        rows = lambda k: body[HDR:HDR + k * ROW].reshape(k, ROW)[:, :64].copy().view(np.uint64)
        return body, rows, [int(bs[r].x) for r in range(R)], arena
    body, rows, xs, _a = call(())
    assert [int(v) for v in body[:16].view(np.uint32)] == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
    assert rows(R)[:, 0].tolist() == xs
    body, rows, xs, _a = call({7})
    assert [int(v) for v in body[:16].view(np.uint32)] == [L.TABLE_MAGIC, L.lib.dpm_version(), R, 1]
    assert rows(R - 1)[:, 0].tolist() == [x for r, x in enumerate(xs) if r != 7]
    assert bool((body[HDR + (R - 1) * ROW:] == 0xAB).all())
    # flag four of them: the sixteen left are a kernarg group again and write no rows at all
    body, rows, xs, _a = call({0, 7, 8, 19})
    assert [int(v) for v in body[:16].view(np.uint32)][2:] == [R, 0] and bool((body[HDR:] == 0xAB).all())


# ------------------------------------------------------------------------------------------------
# WrappedModel.__call__ and the double against the published expression
# ------------------------------------------------------------------------------------------------
def _diffusers(noise_cfg, noise_pred_text, guidance_rescale):
    """rescale_noise_cfg of diffusers' pipelines (Lin et al. 2023, section 3.4), literally"""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("phi,scale", [(0.7, 7.5), (1.0, 1.5)])
def test_call_matches_the_diffusers_expression(monkeypatch, model_type, phi, scale):
    """fp32 torch at [3,4,8,8]: the wrapper's float64 statistics against diffusers' fp32 ones.  Bar: the project's 1e-5 of
    the tensor's scale.  Measured worst case over the four cases: 6.3e-8 (noise network, phi 1, scale 1.5: one fp32 rounding of
    the ratio; 0 at phi 0.7, scale 7.5)."""
    RD.install_rescale_double(monkeypatch, S, D)
    ns = make_schedule("sd")
    fn0, _ = _wrapper(model_type, scale, ns=ns)
    c = torch.tensor([1.0, 2.0, 3.0])
    fn0.condition, fn0.unconditional_condition = c, c * 0
    fn = D.cfg_rescale(fn0, phi)
    x = torch.randn(3, 4, 8, 8, generator=torch.Generator().manual_seed(5))
    t = torch.tensor([0.9, 0.5, 0.1])
    got = fn(x, t)
    e0, e1, _ = fn.raw_outputs(x, t)
    raw = _diffusers(e1 + scale * (e0 - e1), e0, phi)
    if model_type == "v":
        a, s = ns.marginal_alpha(t).reshape(-1, 1, 1, 1), ns.marginal_std(t).reshape(-1, 1, 1, 1)
        want = a * raw + s * x
    else:
        want = raw
    err = float((got - want).abs().max() / want.abs().max())
    print("cfg_rescale __call__ vs diffusers, %s phi=%g scale=%g: %.3g of the scale" % (model_type, phi, scale, err))
    assert got.dtype is torch.float32 and err <= 1e-5
    # phi = 0: the reference's own expression, bit for bit
    assert torch.equal(D.cfg_rescale(fn0, 0.0)(x, t), fn0(x, t))


@pytest.mark.parametrize("ed", [torch.float32, torch.float16, torch.bfloat16])
def test_double_restates_the_contract_and_its_inputs_are_decidable(ed):
    """the numpy double against an independent float64 evaluation of the formula (1e-6 of the scale: fp32 roundings only),
    and the precondition holds for the seeds the GPU tests use"""
    import kernel_double as KD
    rng = np.random.default_rng(11)
    B, P = 3, 4100
    st, _, _ = _record(form=L.FORM_LIN1, flags=L.F_CFG_RESCALE, phi=0.7)
    rnd = KD.half_rounder(ed) or (lambda a: a)
    e0, e1 = (rnd(rng.standard_normal(B * P).astype(np.float32)) for _ in range(2))
    x = rng.standard_normal(B * P).astype(np.float32)
    RD.assert_inputs_decidable(st, e0, e1, B, ed)
    out, mn = RD.stage(st, x, x, e0, e1, None, None, B, ed)
    c, u = e0.astype(np.float64).reshape(B, P), e1.astype(np.float64).reshape(B, P)
    g = rnd(u + 7.5 * (c - u)) if ed is not torch.float32 else u + np.float64(np.float32(7.5)) * (c - u)
    g = np.asarray(g, dtype=np.float64)
    f = c.std(axis=1, ddof=1, keepdims=True) / g.std(axis=1, ddof=1, keepdims=True)
    phi = np.float64(np.float32(0.7))
    want = (phi * (g * f) + (1 - phi) * g).reshape(-1)
    tol = {torch.float32: 1e-6, torch.float16: 2e-3, torch.bfloat16: 2e-2}[ed]     # the half blend rounds three times
    assert float(np.abs(mn - want).max() / np.abs(want).max()) <= tol
    assert np.array_equal(out, (np.float32(0.9) * x - np.float32(-0.1) * mn).astype(np.float32))
    # a constant sample: f = 0 / 0, every element NaN; the others unaffected
    e0[:P] = e1[:P] = np.float32(0.25)
    out2, _ = RD.stage(st, x, x, e0, e1, None, None, B, ed)
    assert np.isnan(out2[:P]).all() and np.array_equal(out2[P:], out[P:])
