"""Perp-Neg guidance (dpm_solver_amd.cfg_perp_neg, DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 stage; C ABI version 220) without a GPU:
the helper, its identity setting and every refusal in both orders, the stage records the binder builds (the kernels replaced by
the numpy double, tests/perp_double.py), the cache keys, the argument errors dpm_stage_launch decides before it touches HIP --
each new one and its turn among the existing ones --, the three anchors of the contract on the double, the torch statement
against the double, and sample() on the double against a torch float64 restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import kernel_double as KD
import perp_double as PP
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule

CFG, PAIR = L.GUIDE["classifier-free"], L.GUIDE["classifier-free-2"]
PERP = L.F_CFG2_PERP
F32 = np.float32


class Net:
    """a network whose output depends on x, t and the per-sample condition, not linearly in the condition (so that the negative
    direction is neither parallel nor perpendicular to the positive one); records the batch of every call"""

    def __init__(self):
        self.calls = []

    def __call__(self, x, t, c):
        self.calls.append(int(x.shape[0]))
        cc = c.reshape(-1, 1, 1, 1).to(x.dtype)
        return (torch.tanh(x * 0.7) * (0.5 + 0.1 * cc) + 0.05 * x + 0.2 * cc * torch.cos(3.0 * x * cc)
                + 0.01 * t.reshape(-1, 1, 1, 1).to(x.dtype))


def _wrapper(model_type="noise", scale=3.0, uncond=True, net=None, ns=None):
    ns = ns or make_schedule("sd")
    c = torch.ones(2)
    return D.model_wrapper(net or Net(), ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=scale,
                           condition=c, unconditional_condition=c * 0 if uncond else None), ns


NEG = torch.full((2,), -0.5)


def _solver(w=1.5, algorithm_type="dpmsolver++", **kw):
    wkw = {k: kw.pop(k) for k in ("model_type", "scale", "net") if k in kw}
    fn, ns = _wrapper(**wkw)
    return D.DPM_Solver(fn if w is None else D.cfg_perp_neg(fn, NEG, w), ns, algorithm_type=algorithm_type, **kw)


def _x(seed=0):
    return torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------
def test_abi_220_value_and_binding():
    assert L.lib.dpm_version() >= 220 and PERP == 8192
    assert C.sizeof(L.Stage) == L.lib.dpm_sizeof(0) and C.sizeof(L.Buffers) == L.lib.dpm_sizeof(1)
    assert "cfg_perp_neg" in D.__all__ and len(L.SYMBOLS) == 62           # no struct grew, no entry point was added
    assert PERP & (L.F_CFG_RESCALE | L.F_CFG_APG | L.F_CFG_ZSTAR | L.F_STORE_XC | L.F_UNIPC_DP | L.F_UNIPC_P2) == 0


def test_helper_returns_a_copy_with_the_marker_set():
    fn, _ = _wrapper()
    assert fn.guidance_perp is False and not fn.perp
    out = D.cfg_perp_neg(fn, NEG)                                           # neg_scale defaults to 1
    assert isinstance(out, D.WrappedModel) and out is not fn and fn.guidance_pair is None and not fn.perp
    assert out.model is fn.model and out.condition is fn.condition and out.guidance_scale == fn.guidance_scale
    assert out.perp and out.pair[0] is NEG and out.pair[1:] == (3.0, 1.0) and out.effective_guidance == "classifier-free-2"
    assert D.cfg_perp_neg(fn, NEG, 0.25).pair[1:] == (3.0, 0.25) and D.cfg_perp_neg(fn, NEG, -2).pair[1:] == (3.0, -2.0)
    one = D.cfg_perp_neg(_wrapper(scale=1.0)[0], NEG, 1.5)                  # the negative still guides at guidance_scale == 1
    assert one.perp and one.effective_guidance == "classifier-free-2"
    # cfg_pair's wrappers carry no marker
    assert not D.cfg_pair(fn, NEG, 1.5).perp


def test_a_zero_negative_scale_is_a_plain_copy_and_evaluates_no_third_branch(monkeypatch):
    PP.install_perp_double(monkeypatch, S, D)
    x = _x(1)
    net = Net()
    plain = _solver(None, net=net).sample(x, steps=4, order=2)
    for w in (0.0, -0.0, 0):
        net2 = Net()
        dpm = _solver(w, net=net2)
        wr = dpm._wrapped
        assert wr.pair is None and wr.guidance_pair is None and not wr.perp and wr.effective_guidance == "classifier-free"
        assert dpm._pair_key() is None and not dpm._perp()
        assert torch.equal(dpm.sample(x, steps=4, order=2), plain)
        assert net2.calls == net.calls == [4] * len(net.calls)                # 2B, never 3B


def test_helper_validation():
    ns = make_schedule("sd")
    for bad in (lambda x, t: x, D.model_wrapper(lambda x, t: x, ns), D.model_wrapper(
            lambda x, t: x, ns, guidance_type="classifier", classifier_fn=lambda *a: 0, condition=torch.ones(1))):
        with pytest.raises(ValueError, match="cfg_perp_neg: takes the result of model_wrapper\\(..., guidance_type='classifier-free'\\)"):
            D.cfg_perp_neg(bad, NEG, 1.0)
    with pytest.raises(ValueError, match="cfg_perp_neg: takes a classifier-free wrapper with an unconditional_condition"):
        D.cfg_perp_neg(_wrapper(uncond=False)[0], NEG, 1.0)
    fn, _ = _wrapper()
    for bad in (float("nan"), float("inf"), -float("inf"), True, "1.5", None):
        with pytest.raises(ValueError, match="cfg_perp_neg: neg_scale must be a finite real number"):
            D.cfg_perp_neg(fn, NEG, bad)
    with pytest.raises(ValueError, match="cfg_perp_neg: negative_condition must be a tensor"):
        D.cfg_perp_neg(fn, [0.0, 0.0], 1.0)
    with pytest.raises(ValueError, match="cfg_perp_neg: negative_condition has shape \\(3,\\)"):
        D.cfg_perp_neg(fn, torch.zeros(3), 1.0)
    with pytest.raises(ValueError, match="cfg_perp_neg: the wrapper's guidance_scale must be a finite real number"):
        D.cfg_perp_neg(_wrapper(scale=float("nan"))[0], NEG, 1.0)


def test_perp_neg_and_the_other_helpers_refuse_each_other_in_either_order():
    fn, _ = _wrapper()
    p = D.cfg_perp_neg(fn, NEG, 1.5)
    for name, make in (("cfg_rescale", lambda f: D.cfg_rescale(f, 0.7)), ("cfg_apg", lambda f: D.cfg_apg(f, 0.5)),
                       ("cfg_zero_star", D.cfg_zero_star), ("cfg_pair", lambda f: D.cfg_pair(f, NEG, 0.5))):
        with pytest.raises(NotImplementedError, match="cfg_perp_neg on top of %s: " % name):
            D.cfg_perp_neg(make(fn), NEG, 1.5)
        with pytest.raises(NotImplementedError, match="%s on top of cfg_perp_neg: " % name):
            make(p)
    with pytest.raises(NotImplementedError, match="cfg_perp_neg on top of cfg_perp_neg: "):
        D.cfg_perp_neg(p, NEG, 0.5)
    # the existing messages are what they were
    q = D.cfg_pair(fn, NEG, 1.5)
    with pytest.raises(NotImplementedError, match="cfg_zero_star on top of cfg_pair: the two-condition stage kernel has no remedy"):
        D.cfg_zero_star(q)
    with pytest.raises(NotImplementedError, match="cfg_pair on top of cfg_apg: the two-condition stage kernel has no remedy"):
        D.cfg_pair(D.cfg_apg(fn, 0.5), NEG, 1.5)
    # the identities refuse nothing, in either order
    assert D.cfg_rescale(p, 0.0).perp and D.cfg_apg(p, 1.0, 0.0, 0.0).perp
    assert D.cfg_perp_neg(D.cfg_rescale(fn, 0.0), NEG, 1.5).perp and D.cfg_perp_neg(D.cfg_pair(fn, NEG, 0.0), NEG, 1.5).perp


def test_raw_outputs_is_one_call_on_three_copies():
    net = Net()
    fn = D.cfg_perp_neg(_wrapper(net=net)[0], NEG, 1.5)
    x = _x(2)
    t = torch.full((2,), 0.5)
    e0, e1, e2 = fn.raw_outputs(x, t)
    assert net.calls == [6]
    ti = fn.get_model_input_time(t)
    lone = Net()
    assert torch.equal(e0, lone(x, ti, torch.ones(2))) and torch.equal(e1, lone(x, ti, torch.zeros(2)))
    assert torch.equal(e2, lone(x, ti, NEG))


# ------------------------------------------------------------------------------------------------
# the refusals of the pair plumbing apply unchanged; the pools
# ------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(monkeypatch):
    PP.install_perp_double(monkeypatch, S, D)
    x = _x()
    dpm = _solver()
    P = "guidance over two conditions \\(cfg_pair\\): "
    with pytest.raises(NotImplementedError, match=P + "sample_sde"):
        dpm.sample_sde(x, steps=6, seed=1)
    with pytest.raises(NotImplementedError, match=P + "sample_unipc"):
        dpm.sample_unipc(x, steps=6)
    with pytest.raises(NotImplementedError, match=P + "correcting_x0_fn='dynamic_thresholding'"):
        _solver(correcting_x0_fn="dynamic_thresholding").sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match=P + "a callable correcting_x0_fn"):
        _solver(correcting_x0_fn=lambda x0, t: x0.clamp(-1, 1)).sample(x, steps=6, order=2)
    blend = D.MaskBlend(make_schedule("sd"), torch.ones(8, 8), x0=x, noise=x)
    with pytest.raises(NotImplementedError, match=P + "a MaskBlend corrector"):
        _solver(correcting_xt_fn=blend).sample(x, steps=6, order=2)
    with pytest.raises(NotImplementedError, match="request_pool: pair=True with a cfg_perp_neg wrapper .*a follow-up"):
        dpm.request_pool(slots=8, pair=True)
    with pytest.raises(NotImplementedError, match=P + "request_pool"):
        dpm.request_pool(slots=8)
    with pytest.raises(NotImplementedError, match=P + "correcting_x0_fn='dynamic_thresholding'"):
        _solver(correcting_x0_fn="dynamic_thresholding").request_pool()
    # cfg_pair's own pool rules are what they were
    fn, ns = _wrapper()
    with pytest.raises(NotImplementedError, match=P + "request_pool"):
        D.DPM_Solver(D.cfg_pair(fn, NEG, 1.5), ns, algorithm_type="dpmsolver++").request_pool()
    # a Python correcting_xt_fn, return_intermediate and denoise_to_zero are supported
    out, inter = _solver(correcting_xt_fn=lambda xt, t, step: xt * 0.999).sample(x, steps=4, order=2, denoise_to_zero=True,
                                                                               return_intermediate=True)
    assert torch.isfinite(out).all() and len(inter) == 6


def test_a_request_pool_without_slots_takes_the_solver_as_it_is(monkeypatch):
    PP.install_perp_double(monkeypatch, S, D)
    dpm = _solver()
    xs = [_x(3), _x(4)]
    want = [dpm.sample(x, steps=4, order=2) for x in xs]
    pool = dpm.request_pool()
    hs = [pool.submit(x, steps=4, order=2) for x in xs]
    done = {}
    for _ in range(8):
        done.update(pool.step())
    assert set(done) == set(hs) and all(torch.equal(done[h], w) for h, w in zip(hs, want))


# ------------------------------------------------------------------------------------------------
# the records, the keys
# ------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """the stage records that reach the launch entry points, as (flags, cfg_scale, cg_scale, guidance) in call order"""
    PP.install_perp_double(monkeypatch, S, D)
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
def test_binder_sets_the_flag_and_w_in_every_record(monkeypatch, algorithm_type, kw):
    seen = _spy(monkeypatch)
    x = _x(1)
    ok = lambda rows: all(f & PERP and s == 3.0 and c == 0.75 and g == PAIR and not f & (L.F_THRESH | L.F_BLEND | L.F_NOISE)
                          for f, s, c, g in rows)
    dpm = _solver(0.75, algorithm_type)
    out = dpm.sample(x, **kw)                                               # the prebuilt records (fast path)
    assert seen and ok(seen) and torch.isfinite(out).all()
    n_fast = len(seen)
    out_i, inter = dpm.sample(x, return_intermediate=True, **kw)            # the general loop binds the same records
    assert len(seen) == 2 * n_fast and ok(seen[n_fast:]) and torch.equal(out, out_i)
    del seen[:]
    outs = dpm.sample_requests([x, x + 1], **kw)                            # one multi-request call per stage
    assert len(seen) == 2 * n_fast and ok(seen) and torch.equal(outs[0], out)
    assert not torch.equal(out, _solver(None, algorithm_type).sample(x, **kw))
    # cfg_pair with the same tensor and scales: records without the flag, another result
    del seen[:]
    fn, ns = _wrapper()
    lin = D.DPM_Solver(D.cfg_pair(fn, NEG, 0.75), ns, algorithm_type=algorithm_type)
    assert not torch.equal(lin.sample(x, **kw), out) and seen and not any(f & PERP for f, s, c, g in seen)


def test_cache_keys_change_with_the_setting_and_are_unchanged_without_it(monkeypatch):
    seen = _spy(monkeypatch)
    x = _x(3)
    dpm = _solver(1.5)
    w = dpm._wrapped
    k0 = dpm._pair_key()
    assert k0 == (id(NEG), 3.0, 1.5, "perp_neg")
    a = dpm.sample(x, steps=4, order=2)
    n, plans = len(seen), len(dpm._plans)
    w.guidance_perp = False                                                  # the same triple as cfg_pair's: another key,
    k1 = dpm._pair_key()                                                     # other records, another plan entry
    b = dpm.sample(x, steps=4, order=2)
    assert k1 == (id(NEG), 3.0, 1.5) and len(dpm._plans) == plans + 1 and len(dpm._fast) == 2
    assert all(f & PERP for f, s, c, g in seen[:n]) and not any(f & PERP for f, s, c, g in seen[n:])
    assert not torch.equal(a, b)
    # ... which is the key cfg_pair's own wrapper has: without cfg_perp_neg every key equals what it was
    fn, ns = _wrapper()
    lin = D.DPM_Solver(D.cfg_pair(fn, NEG, 1.5), ns, algorithm_type="dpmsolver++")
    assert lin._pair_key() == (id(NEG), 3.0, 1.5) and D.DPM_Solver(fn, ns)._pair_key() is None
    w.guidance_perp = True
    c2, s, _ = w.guidance_pair
    w.guidance_pair = (c2, s, 2.5)                                           # another negative scale: another key
    assert dpm._pair_key() == (id(NEG), 3.0, 2.5, "perp_neg")
    c = dpm.sample(x, steps=4, order=2)
    assert [cg for f, s_, cg, g in seen[2 * n:]] == [2.5] * n and not torch.equal(a, c)


# ------------------------------------------------------------------------------------------------
# the C side, before HIP
# ------------------------------------------------------------------------------------------------
def _record(form=L.FORM_TWO, flags=L.F_TO_X0 | L.F_STORE_M | PERP, guidance=PAIR, s=7.5, w=1.5, n=64, batch=2, dtype=L.DTYPE_F32):
    """a well-formed flagged request on CPU pointers (never read: the calls below end before any launch)"""
    arena = np.zeros(10 * n * 8 + 64, dtype=np.uint8)
    base = (arena.ctypes.data + 63) // 64 * 64
    st, b = L.Stage(), L.Buffers()
    st.form, st.flags, st.guidance, st.model_type = form, flags, guidance, L.MODEL["noise"]
    st.alpha_e, st.sigma_e, st.cfg_scale, st.cg_scale = 0.8, 0.6, s, w
    st.cx, st.c0, st.c1 = 0.9, -0.1, 0.05
    st.h1_slot = st.h2_slot = st.m_slot = -1
    p = [base + k * n * 8 for k in range(10)]
    b.x, b.e0, b.e1, b.g, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]
    b.n, b.batch, b.state_dtype, b.eps_dtype = n, batch, dtype, dtype
    return st, b, arena


TX = L.F_TO_X0 | PERP
SPLIT = "stage_launch: DPM_GUIDE_CFG2 with thresholding, mask blend, noise or a split stage (flags %d)"
ONLY = "stage_launch: DPM_F_CFG2_PERP is valid under DPM_GUIDE_CFG2 only (guidance %d)"
BATCH = "stage_launch: DPM_F_CFG2_PERP with a batch of %d (one workgroup per sample)"
TEXTS = [   # every refusal of a flagged record, in the order dpm_stage_launch asks: return code and the whole message
    (dict(guidance=CFG), L.ERR_ARG, ONLY % CFG),
    (dict(guidance=L.GUIDE["uncond"]), L.ERR_ARG, ONLY % 0),
    (dict(guidance=L.GUIDE["classifier"]), L.ERR_ARG, ONLY % 2),
    (dict(n=1 << 32, batch=1 << 31), L.ERR_UNSUPPORTED, BATCH % (1 << 31)),
    # the existing checks keep their texts and their turn: the remedy flags first, then DPM_GUIDE_CFG2's own, then the flag's
    (dict(flags=TX | L.F_CFG_RESCALE), L.ERR_ARG, "stage_launch: DPM_F_CFG_RESCALE is valid under classifier-free guidance only (guidance 3)"),
    (dict(flags=TX | L.F_CFG_APG), L.ERR_ARG, "stage_launch: DPM_F_CFG_APG is valid under classifier-free guidance only (guidance 3)"),
    (dict(flags=TX | L.F_CFG_ZSTAR), L.ERR_ARG, "stage_launch: DPM_F_CFG_ZSTAR is valid under classifier-free guidance only (guidance 3)"),
    (dict(flags=TX | L.F_CFG_ZSTAR, guidance=CFG), L.ERR_ARG, ONLY % CFG),            # (the remedy's checks pass; then the flag's)
    (dict(s=float("nan")), L.ERR_ARG,
     "stage_launch: DPM_GUIDE_CFG2 with s1=nan (dpm_stage.cfg_scale), s2=1.5 (dpm_stage.cg_scale): both must be finite"),
    (dict(w=float("inf")), L.ERR_ARG,
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
    (dict(n=1 << 32, batch=1 << 31, dtype=L.DTYPE_F64), L.ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with a double state (no double kernel)"),
    (dict(n=1 << 32, batch=1 << 31, null="g"), L.ERR_UNSUPPORTED, BATCH % (1 << 31)),
    (dict(guidance=CFG, null="e1"), L.ERR_ARG, ONLY % CFG),
    (dict(guidance=CFG, form=6), L.ERR_ARG, ONLY % CFG),
    (dict(guidance=CFG, n=1 << 32, batch=1 << 31), L.ERR_ARG, ONLY % CFG),
]


@pytest.mark.parametrize("kw,code,text", TEXTS, ids=[str(i) for i in range(len(TEXTS))])
def test_every_refusal_has_its_code_its_text_and_its_turn(kw, code, text):
    kw = dict(kw)
    stride, null, xo2 = kw.pop("stride", 0), kw.pop("null", None), kw.pop("x_out2", False)
    st, b, arena = _record(**{k: v for k, v in kw.items() if k not in ("n", "batch")})
    if "n" in kw:
        b.n, b.batch = kw["n"], kw["batch"]                     # (one element per sample; nothing is read)
    b.eps_stride = stride
    if null:
        setattr(b, null, None)
    if xo2:
        b.x_out2 = b.m_out + 8 * 64
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


def test_the_unflagged_record_meets_the_lines_it_met():
    """the pinned cases of tests/test_cfg_pair_host.py run in that file; here: a record that differs from a refused flagged one
    in the flag alone is refused by the same line"""
    for kw in (dict(s=float("nan")), dict(form=L.FORM_UNIPC), dict(dtype=L.DTYPE_F64), dict(form=6)):
        st, b, _ = _record(**kw)
        rc = L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None)
        text = L.lib.dpm_last_error()
        st.flags &= ~PERP
        assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == rc and L.lib.dpm_last_error() == text


@pytest.mark.parametrize("extra", [0, L.TABLE_PAIR, L.TABLE_PAIR | L.TABLE_ZSTAR | L.TABLE_NOISE])
@pytest.mark.parametrize("mode", [L.TABLE_FILL, L.TABLE_LAUNCH])
def test_a_table_mode_call_refuses_the_flag_and_writes_nothing(mode, extra):
    ok_st, ok_b, arena0 = _record(flags=L.F_TO_X0 | L.F_STORE_M)
    st, b, arena1 = _record()
    opts = L.LaunchOpts()
    opts.per_request_stages, opts.table_mode = 1, mode | extra
    table = np.full(L.table_bytes(2, extra) + 16, 0xAB, dtype=np.uint8)
    ok_b.workspace = table.ctypes.data + (-table.ctypes.data) % 16
    ok_b.opts = C.pointer(opts)
    bs = (L.Buffers * 2)(ok_b, b)
    assert L.lib.dpm_stage_launch_multi((L.Stage * 2)(ok_st, st), bs, 2, None) == L.ERR_UNSUPPORTED
    assert L.lib.dpm_last_error().decode() == ("stage_launch_multi: DPM_F_CFG2_PERP in a table-mode call (the table's rows have "
                                                "no per-sample pass)")
    assert bool((table == 0xAB).all()) and not arena0.any() and not arena1.any()
    # the record's own errors come first
    st.cg_scale = float("nan")
    assert L.lib.dpm_stage_launch_multi((L.Stage * 2)(ok_st, st), bs, 2, None) == L.ERR_ARG
    assert b"both must be finite" in L.lib.dpm_last_error()


def test_device_resident_coefficients_are_refused_as_for_the_guidance():
    st, b, arena = _record()
    handle = np.zeros(1 << 16, dtype=np.uint8)
    assert L.lib.dpm_adaptive_stage_launch(handle.ctypes.data, 1, C.byref(st), C.byref(b), None) == L.ERR_UNSUPPORTED
    assert L.lib.dpm_last_error().decode() == "stage_launch: DPM_GUIDE_CFG2 with device-resident coefficients"
    assert not arena.any() and not handle.any()


def test_an_empty_batch_is_ok_and_its_record_is_still_checked():
    st, b, _ = _record(n=0, batch=1)
    b.e1 = b.g = None                                       # (nothing would be read)
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == 0
    st.guidance = CFG
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(b), None) == L.ERR_ARG


def test_the_planner_never_sets_the_flag():
    dpm = _solver(1.5)
    ns = dpm.noise_schedule
    for method, order in (("multistep", 3), ("singlestep", 3)):
        plan = dpm._get_plan(method=method, order=order, steps=6, skip_type="time_uniform", solver_type="dpmsolver",
                             lower_order_final=True, denoise_to_zero=True, t_T=ns.T, t_0=1.0 / ns.total_N)
        assert all(a.guidance == PAIR and not a.flags & PERP and a.cg_scale == 0.0 for a in plan.stages)


# ------------------------------------------------------------------------------------------------
# the double: the contract in float64, the three anchors bit for bit
# ------------------------------------------------------------------------------------------------
def _gd64(oc, ou, on, s, w):
    d0, d2 = oc - ou, on - ou
    s_dd = (d0 * d0).sum(axis=1, keepdims=True)
    a = np.where(s_dd > 0, (d2 * d0).sum(axis=1, keepdims=True) / np.where(s_dd > 0, s_dd, 1.0), 0.0)
    return ou + s * (d0 - w * (d2 - a * d0))


@pytest.mark.parametrize("ed", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("model_type", ["noise", "x_start", "v", "score"])
def test_double_restates_the_contract(ed, model_type):
    """the numpy double against a float64 evaluation of the formula: 1e-6 of the scale -- a handful of fp32 roundings, a rounded
    once (2^-24 relative on a term of the size of d0); nothing is rounded to the network's dtype after the loads"""
    rng = np.random.default_rng(11)
    B, P = 3, 1367
    n = B * P
    st, _, _ = _record(form=L.FORM_LIN1, flags=PERP)
    st.model_type = L.MODEL[model_type]
    rnd = KD.half_rounder(ed) or (lambda a: a)
    e0, e1, z = (rnd(rng.standard_normal(n).astype(F32)) for _ in range(3))
    e2 = rnd((e1 + 0.8 * (e0 - e1) + 0.6 * z).astype(F32))
    x = rng.standard_normal(n).astype(F32)
    PP.assert_inputs_decidable(e0, e1, e2, B)
    out, mn = PP.stage(st, x, x, e0, e1, e2, None, None, B)
    a = PP.projection(*(e.reshape(B, P) for e in (e0, e1, e2)))
    assert np.all(np.abs(a - 0.8) < 0.1)
    gd = _gd64(*(e.astype(np.float64).reshape(B, P) for e in (e0, e1, e2)), 7.5, 1.5).reshape(n)
    want = KD.to_noise(gd, x.astype(np.float64), KD._Coef(st, np.float64))
    assert float(np.abs(mn - want).max() / np.abs(want).max()) <= 1e-6
    assert np.array_equal(out, (F32(0.9) * x - F32(-0.1) * mn).astype(F32))


@pytest.mark.parametrize("w", [1.5, -0.25])
def test_the_three_anchors_on_the_double(w):
    rng = np.random.default_rng(13)
    B, P = 2, 4100
    n = B * P
    st, _, _ = _record(form=L.FORM_DENOISE, flags=PERP | L.F_STORE_M, w=w)     # noise network, no conversion: x_out = mn = gd
    e0, e1, e2 = (rng.standard_normal(n).astype(F32) for _ in range(3))
    x = rng.standard_normal(n).astype(F32)
    s, w32 = F32(7.5), F32(w)
    d0 = (e0 - e1).astype(F32)
    cfg = (e1 + (s * d0).astype(F32)).astype(F32)                            # o_u + s * d0
    # g == e0: d2 == d0 bit for bit, a = S / S = 1, perp = d0 - 1 * d0 = 0, d0 - w * 0 = d0
    assert np.array_equal(PP.projection(*(e.reshape(B, P) for e in (e0, e1, e0))), np.ones(B, F32))
    assert np.array_equal(PP.stage(st, x, x, e0, e1, e0, None, None, B)[0], cfg)
    # g == e1: d2 = 0, a = 0, perp = 0 - 0 * d0 = 0
    assert np.array_equal(PP.projection(*(e.reshape(B, P) for e in (e0, e1, e1))), np.zeros(B, F32))
    assert np.array_equal(PP.stage(st, x, x, e0, e1, e1, None, None, B)[0], cfg)
    # e0 == e1: d0 = 0, S_dd = 0, a = 0 (defined), gd = o_u + s * (0 - w * d2)
    d2 = (e2 - e1).astype(F32)
    want = (e1 + (s * (F32(0) - (w32 * d2).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    assert np.array_equal(PP.projection(*(e.reshape(B, P) for e in (e1, e1, e2))), np.zeros(B, F32))
    assert np.array_equal(PP.stage(st, x, x, e1, e1, e2, None, None, B)[0], want)
    # ... and none of the three is the general case
    assert not np.array_equal(PP.stage(st, x, x, e0, e1, e2, None, None, B)[0], cfg)


# ------------------------------------------------------------------------------------------------
# the torch statement and sample() against float64
# ------------------------------------------------------------------------------------------------
def _perp64(w, x, t, s, wn, neg):
    """the contract in torch float64 on a float64 x: projection and blend on the raw outputs, the conversion afterwards"""
    ns = w.noise_schedule
    ti = w.get_model_input_time(t)
    oc, ou, on = (w.model(x, ti, c.to(x.dtype)) for c in (w.condition, w.unconditional_condition, neg))
    al, sg = (v.reshape(-1, 1, 1, 1).double() for v in (ns.marginal_alpha(t), ns.marginal_std(t)))
    d0, d2 = oc - ou, on - ou
    a = (d2 * d0).sum(dim=(1, 2, 3), keepdim=True) / (d0 * d0).sum(dim=(1, 2, 3), keepdim=True)
    o = ou + s * (d0 - wn * (d2 - a * d0))
    return {"noise": lambda: o, "x_start": lambda: (x - al * o) / sg, "v": lambda: al * o + sg * x, "score": lambda: -sg * o}[w.model_type]()


@pytest.mark.parametrize("model_type", ["noise", "v", "x_start", "score"])
def test_call_is_the_torch_statement_and_equals_the_double(monkeypatch, model_type):
    PP.install_perp_double(monkeypatch, S, D)
    fn, ns = _wrapper(model_type=model_type, scale=7.5)
    w = D.cfg_perp_neg(fn, NEG, 1.5)
    x = _x(5)
    t = torch.full((2,), 0.6)
    got = w(x, t)
    assert got.dtype is torch.float32
    want = _perp64(w, x.double(), t, 7.5, 1.5, NEG)
    assert float((got.double() - want).abs().max() / want.abs().max()) <= 1e-6
    # ... and a one-stage DENOISE launch of the double gives the same values: equal bits for a noise network (the same fp32
    # operations in the same order), 1e-6 where the conversion's scalars are formed on either side
    dpm = D.DPM_Solver(w, ns, algorithm_type="dpmsolver")
    stage = dpm.noise_prediction_fn(x, torch.tensor([0.6]))
    if model_type == "noise":
        assert torch.equal(stage, got)
    assert float((stage.double() - want).abs().max() / want.abs().max()) <= 1e-6
    # half outputs are widened first and nothing is rounded to half
    half = D.cfg_perp_neg(D.model_wrapper(lambda xx, tt, c: Net()(xx, tt, c).half(), ns, model_type=model_type,
                                          guidance_type="classifier-free", guidance_scale=7.5, condition=torch.ones(2),
                                          unconditional_condition=torch.zeros(2)), NEG, 1.5)
    gh = half(x, t)
    assert gh.dtype is torch.float32 and float((gh.double() - want).abs().max() / want.abs().max()) <= 1e-2


@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("algorithm_type,kw", [("dpmsolver++", dict(steps=6, order=2)), ("dpmsolver", dict(steps=6, order=3)),
                                               ("dpmsolver++", dict(steps=6, order=3, method="singlestep")),
                                               ("dpmsolver++", dict(steps=5, order=2, denoise_to_zero=True))],
                         ids=["2M++", "3M", "3S++", "2M++dz"])
def test_sample_on_the_double_against_a_torch_float64_statement(monkeypatch, model_type, algorithm_type, kw):
    """sample() under cfg_perp_neg, fp32 state, kernels replaced by the numpy double -- against the SAME sampler in float64 on a
    model callable that projects and blends the three branches in torch float64 (what a caller has to write without the
    helper).  The bar is the project's parity bar, 1e-5 of the tensor's scale."""
    PP.install_perp_double(monkeypatch, S, D)
    x = _x(7)
    dpm = _solver(1.5, algorithm_type, model_type=model_type)
    got = dpm.sample(x, **kw)
    w, ns = dpm._wrapped, dpm.noise_schedule
    ref = D.DPM_Solver(lambda xx, tt: _perp64(w, xx, tt, 3.0, 1.5, NEG), ns, algorithm_type=algorithm_type)
    want = ref.sample(x.double(), **kw)
    assert want.dtype is torch.float64 and got.dtype is torch.float32
    assert float((got.double() - want).abs().max() / want.abs().max()) <= 1e-5
    # a double state: the three outputs are projected and blended in torch, in double, and the stage is unguided
    got64 = dpm.sample(x.double(), **kw)
    assert got64.dtype is torch.float64 and float((got64 - want).abs().max() / want.abs().max()) <= 1e-12
    outs64 = dpm.sample_requests([x.double(), x.double() + 1], **kw)
    assert torch.equal(outs64[0], got64)
