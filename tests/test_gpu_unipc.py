"""UniPC on the MI355X: one DPM_FORM_UNIPC launch per route against the fp32 numpy double of the stage, bit for bit;
sample_unipc trajectories against the float64 restatement of the published update and against the double; channels_last,
graph capture, the plain-C loops and a per-request-stage launch with a UniPC stage among ODE stages."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import unipc_double as UD
import kernel_double as KD
import test_unipc_host as H
from dpm_solver_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_DT = {torch.float32: L.DTYPE_F32, torch.float16: L.DTYPE_F16, torch.bfloat16: L.DTYPE_BF16}
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float16, torch.float16),
         (torch.bfloat16, torch.bfloat16)]
SHAPES = [(False, False), (False, True), (True, False), (True, True)]      # (second-order corrector, second-order predictor)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _stage(dp, p2, guidance="uncond", model="noise", index=3, alpha=0.8, seed=0):
    """a UniPC stage record with scalars of realistic magnitude"""
    r = np.random.default_rng(seed + 17)
    st = L.Stage()
    st.index, st.form, st.model_type, st.guidance = index, L.FORM_UNIPC, L.MODEL[model], L.GUIDE[guidance]
    st.flags = L.F_TO_X0 | L.F_STORE_M | (L.F_UNIPC_DP if dp else 0) | (L.F_UNIPC_P2 if p2 else 0)
    st.h1_slot, st.h2_slot, st.m_slot, st.emits_state = 0, (1 if dp else -1), 2, 1
    st.alpha_e, st.sigma_e = alpha, float(np.sqrt(1 - alpha * alpha))
    st.cfg_scale = 2.5
    st.cx, st.c0, st.c1, st.c2 = 0.83 + 0.01 * r.random(), -0.47 - 0.01 * r.random(), -0.238, -0.208
    st.k[0], st.k[1], st.k[2] = 0.6685, -0.2782, -0.6686
    return st


class _Case:
    """the operands of one launch as CPU tensors (for the double) and, cloned, on the GPU (for the kernel)"""

    def __init__(self, st, n, sdt, edt, batch=2, offset=0, dup=False, xc=False, stride=False, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.st, self.n, self.batch, self.sdt, self.edt = st, n, batch, sdt, edt
        cfg = st.guidance == L.GUIDE["classifier-free"]
        mk = lambda dt, m=n: torch.randn(m + offset, generator=g).to(dt)
        per = n // batch
        self.t = dict(x=mk(sdt), h1=mk(sdt), h2=mk(sdt) if st.flags & L.F_UNIPC_DP else None,
                      e0=mk(edt, 2 * n if stride else n), e1=(mk(edt, 2 * n if stride else n) if cfg else None),
                      x_out=torch.zeros(n + offset).to(sdt), m_out=torch.zeros(n + offset).to(sdt),
                      x_out2=torch.zeros(n + offset).to(sdt) if (dup or xc) else None)
        self.offset, self.stride = offset, (2 * per if stride else 0)
        if xc:
            st.flags |= L.F_STORE_XC

    def buffers(self, tensors, opts=None):
        b = L.Buffers()
        for k, t in tensors.items():
            if t is not None:
                setattr(b, k, t.data_ptr() + self.offset * t.element_size())
        b.n, b.batch = self.n, self.batch
        b.state_dtype, b.eps_dtype = _DT[self.sdt], _DT[self.edt]
        b.eps_stride = self.stride
        if opts is not None:
            b.opts = C.pointer(opts)
        return b

    def expect(self):
        cpu = {k: (None if t is None else t.clone()) for k, t in self.t.items()}
        assert UD.launch_raw_double(KD._Ref(self.st), KD._Ref(self.buffers(cpu)), None) == 0
        return cpu

    def gpu(self):
        return {k: (None if t is None else t.to(DEV)) for k, t in self.t.items()}


def _same(got, want, what):
    for k in ("x_out", "m_out", "x_out2"):
        if want[k] is not None:
            assert torch.equal(got[k].cpu().view(torch.int16 if want[k].element_size() == 2 else torch.int32),
                               want[k].view(torch.int16 if want[k].element_size() == 2 else torch.int32)), (what, k)


def _launch_and_compare(case, what):
    want, dev = case.expect(), case.gpu()
    b = case.buffers(dev)
    L.check(L.lib.dpm_stage_launch(C.byref(case.st), C.byref(b), _stream()))
    torch.cuda.synchronize()
    _same(dev, want, what)
    assert float(want["x_out"].float().abs().max()) > 0.1


@pytest.mark.parametrize("sdt,edt", PAIRS, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("dp,p2", SHAPES)
def test_one_launch_per_route_equals_the_double(sdt, edt, dp, p2):
    n = 2 * 4 * 64 * 64
    tag = (sdt, edt, dp, p2)
    _launch_and_compare(_Case(_stage(dp, p2), n, sdt, edt), ("vector",) + tag)
    _launch_and_compare(_Case(_stage(dp, p2), n + 8 + 3, sdt, edt, batch=1), ("vector + ragged tail",) + tag)
    _launch_and_compare(_Case(_stage(dp, p2), n, sdt, edt, offset=1), ("per-lane, unaligned views",) + tag)
    _launch_and_compare(_Case(_stage(dp, p2, "classifier-free"), n, sdt, edt, dup=True), ("CFG duplicate store",) + tag)
    _launch_and_compare(_Case(_stage(dp, p2), n, sdt, edt, stride=True), ("eps_stride",) + tag)
    _launch_and_compare(_Case(_stage(dp, p2), n, sdt, edt, xc=True), ("corrected-state store",) + tag)
    _launch_and_compare(_Case(_stage(dp, p2), n, sdt, edt, xc=True, offset=1), ("corrected-state store, per-lane",) + tag)
    _launch_and_compare(_Case(_stage(dp, p2, model="v", alpha=0.6), n, sdt, edt), ("general prologue",) + tag)


@pytest.mark.parametrize("dp,p2", [(True, True), (False, False)])
def test_a_launch_above_the_big_tiles_threshold_equals_the_double(dp, p2):
    n = 16384 * 2048                       # DPM_BIG_TILES_DEFAULT tiles: handed to the fused kernel as a group of one
    _launch_and_compare(_Case(_stage(dp, p2), n, torch.float16, torch.float16, batch=4), ("big_tiles", dp, p2))


@pytest.mark.parametrize("sdt,edt", PAIRS, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("n_req", [2, 5, 32])
def test_lockstep_fused_launch_equals_the_double(sdt, edt, n_req):
    n = 4 * 4 * 32 * 32
    for dp, p2 in SHAPES:
        for guidance in ("uncond", "classifier-free"):
            st = _stage(dp, p2, guidance)
            cases = [_Case(st, n, sdt, edt, dup=guidance != "uncond", seed=r) for r in range(n_req)]
            wants, devs = [c.expect() for c in cases], [c.gpu() for c in cases]
            arr = (L.Buffers * n_req)()
            for r, (c, d) in enumerate(zip(cases, devs)):
                arr[r] = c.buffers(d)
            L.check(L.lib.dpm_stage_launch_multi(C.byref(st), arr, n_req, _stream()))
            torch.cuda.synchronize()
            for r in range(n_req):
                _same(devs[r], wants[r], (sdt, edt, n_req, dp, p2, guidance, r))


def test_per_request_stages_with_a_unipc_stage_among_ode_stages():
    """whatever the launch fuses, every request gets the bits of its single launch"""
    n, sdt = 4 * 4 * 32 * 32, torch.float16
    sts = []
    for r in range(6):
        st = _stage(r % 2 == 0, True, seed=r)
        if r in (1, 4):                     # ODE stages of the same plan family: 2M and a first-order stage
            st.form, st.flags = (L.FORM_TWO if r == 1 else L.FORM_LIN1), L.F_TO_X0 | L.F_STORE_M
        sts.append(st)
    cases = [_Case(sts[r], n, sdt, sdt, seed=r) for r in range(6)]
    singles = []
    for c in cases:
        d = c.gpu()
        L.check(L.lib.dpm_stage_launch(C.byref(c.st), C.byref(c.buffers(d)), _stream()))
        singles.append(d)
    opts = L.LaunchOpts()
    opts.per_request_stages = 1
    devs = [c.gpu() for c in cases]
    arr, starr = (L.Buffers * 6)(), (L.Stage * 6)()
    for r, (c, d) in enumerate(zip(cases, devs)):
        arr[r], starr[r] = c.buffers(d, opts), sts[r]
    L.check(L.lib.dpm_stage_launch_multi(starr, arr, 6, _stream()))
    torch.cuda.synchronize()
    for r in range(6):
        for k in ("x_out", "m_out"):
            assert torch.equal(devs[r][k], singles[r][k]), (r, k)
        _same(devs[r], cases[r].expect(), ("het", r))


def test_unsupported_combinations_are_errors():
    c = _Case(_stage(True, True), 2048, torch.float32, torch.float32)
    d = c.gpu()
    for flag, rc in ((L.F_THRESH, L.ERR_UNSUPPORTED), (L.F_BLEND, L.ERR_ARG), (L.F_NOISE, L.ERR_ARG)):
        st = c.st.copy()                    # (blend and noise fail their own operand / form checks first)
        st.flags |= flag
        assert L.lib.dpm_stage_launch(C.byref(st), C.byref(c.buffers(d)), _stream()) == rc
    c64 = _Case(_stage(True, True), 2048, torch.float32, torch.float32)
    b64 = c64.buffers(d)
    b64.state_dtype = b64.eps_dtype = L.DTYPE_F64
    assert L.lib.dpm_stage_launch(C.byref(c64.st), C.byref(b64), _stream()) == L.ERR_UNSUPPORTED     # double states
    st = c.st.copy()
    st.flags |= L.F_STORE_XC
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(c.buffers(d)), _stream()) == L.ERR_ARG      # no x_out2
    st = c.st.copy()
    st.form = L.FORM_TWO
    assert L.lib.dpm_stage_launch(C.byref(st), C.byref(c.buffers(d)), _stream()) == L.ERR_ARG      # UniPC flags elsewhere
    b = c.buffers(d)
    b.h2 = None
    assert L.lib.dpm_stage_launch(C.byref(c.st), C.byref(b), _stream()) == L.ERR_ARG               # second-order corrector


# ---- trajectories ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ns", H._schedules(), ids=lambda v: v if isinstance(v, str) else "")
def test_fp32_trajectories_against_the_float64_restatement(name, ns):
    """<= 1e-5 of the tensor's scale, corrected states one by one and the result.  Worst measured: 6.6e-7 (discrete),
    7.8e-7 (linear); profiles/r11_unipc.md"""
    lam, alpha, sigma = H._sched64(ns)
    x = H._x((2, 4, 16, 16))
    worst = 0.0
    for kind, cfg in H.END_TO_END:
        dpm = D.DPM_Solver(H._engine(kind, ns, None if cfg is None else cfg), ns, algorithm_type="dpmsolver++")
        if cfg is not None:      # the conditioning tensors live where the state lives
            w = dpm._wrapped
            w.condition, w.unconditional_condition = w.condition.to(DEV), w.unconditional_condition.to(DEV)
        for variant in ("bh1", "bh2"):
            for order, steps, skip in ((2, 10, "time_uniform"), (2, 20, "logSNR"), (1, 7, "time_quadratic")):
                kw = dict(steps=steps, order=order, variant=variant, skip_type=skip)
                got, inter = dpm.sample_unipc(x.to(DEV), return_intermediate=True, **kw)
                fast = dpm.sample_unipc(x.to(DEV), **kw)
                assert torch.equal(got, fast)
                grid = H._grid(H._plan(dpm, ns, steps, order, variant, skip))
                want, states = UD.reference_sample(lam, alpha, sigma, grid, H._x0_double(kind, ns, grid, alpha, sigma, cfg),
                                                   x.numpy().astype(np.float64), order, variant)
                assert len(inter) == len(states)
                for g_, w_ in zip(inter + [got], states + [want]):
                    err = float(np.max(np.abs(g_.cpu().numpy() - w_)) / np.max(np.abs(w_)))
                    worst = max(worst, err)
                    assert err <= 1e-5, (name, kind, variant, order, steps, skip, err)
    print("worst scale-relative error on the GPU (%s): %.3g" % (name, worst))


def _cpu_run(fn):
    """fn() with every device entry point on the numpy double"""
    with pytest.MonkeyPatch.context() as mp:
        UD.install_unipc_double(mp, S, D)
        return fn()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_half_trajectories_equal_the_double_bit_for_bit(dt):
    ns = D.NoiseScheduleVP("linear")         # (a half state stays half on a continuous schedule with a noise network)
    net = lambda x, t: (0.5 * x.float() + 0.1 * torch.sin(x.float())).to(x.dtype)
    x = H._x((2, 4, 16, 16)).to(dt)
    for kw in (dict(steps=8), dict(steps=9, variant="bh1", skip_type="logSNR"), dict(steps=6, order=1, denoise_to_zero=True)):
        dpm = D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++")
        want, wi = _cpu_run(lambda: dpm.sample_unipc(x, return_intermediate=True, **kw))
        dpm = D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++")
        got, gi = dpm.sample_unipc(x.to(DEV), return_intermediate=True, **kw)
        assert got.dtype == want.dtype and torch.equal(got.cpu(), want)
        assert len(gi) == len(wi) and all(torch.equal(a.cpu(), b) for a, b in zip(gi, wi))
        assert torch.equal(dpm.sample_unipc(x.to(DEV), **kw).cpu(), want)


def test_channels_last_network_gives_the_same_bits():
    ns = H._discrete()
    net = lambda x, t: 0.5 * x + 0.1 * torch.sin(x)           # elementwise: the same bits in either layout
    x = H._x((2, 4, 16, 16)).to(DEV)
    a = D.DPM_Solver(D.model_wrapper(net, ns), ns).sample_unipc(x, steps=7)
    nhwc = lambda x, t: net(x, t).contiguous(memory_format=torch.channels_last)
    b, bi = D.DPM_Solver(D.model_wrapper(nhwc, ns), ns).sample_unipc(x, steps=7, return_intermediate=True)
    assert torch.equal(a, b) and torch.equal(a, bi[-1]) and len(bi) == 7
    assert torch.equal(a, D.DPM_Solver(D.model_wrapper(nhwc, ns), ns).sample_unipc(x, steps=7))


def test_capture_replay_equals_eager():
    ns = H._discrete()
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: 0.5 * x + 0.1 * torch.sin(x), ns), ns, algorithm_type="dpmsolver++")
    x, y = H._x((2, 4, 16, 16)).to(DEV), H._x((2, 4, 16, 16), 5).to(DEV)
    g = dpm.capture(x, unipc=True, steps=8, variant="bh1")
    assert torch.equal(g(x), dpm.sample_unipc(x, steps=8, variant="bh1"))
    assert torch.equal(g(y), dpm.sample_unipc(y, steps=8, variant="bh1"))


def _run_buffers(xs, E, plan, sdt):
    """dpm_run_buffers of one request with a frozen network output E (model callback NULL)"""
    keep = [xs.clone()] + [torch.empty_like(xs) for _ in range(3)] + [torch.empty_like(xs) for _ in range(plan.slots)]
    rb = L.RunBuffers()
    for i in range(4):
        rb.xbuf[i] = keep[i].data_ptr()
    for i in range(plan.slots):
        rb.hist[i] = keep[4 + i].data_ptr()
    rb.e0 = E.data_ptr()
    rb.n, rb.batch = xs.numel(), xs.shape[0]
    rb.state_dtype = rb.eps_dtype = _DT[sdt]
    return rb, keep


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_plan_run_from_c_equals_sample_unipc(dt):
    ns = D.NoiseScheduleVP("linear")
    E = (0.3 * H._x((2, 4, 16, 16), 7)).to(dt).to(DEV)
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: E, ns), ns, algorithm_type="dpmsolver++")
    xs = [H._x((2, 4, 16, 16), r).to(dt).to(DEV) for r in range(3)]
    want = [dpm.sample_unipc(x, steps=7) for x in xs]
    assert all(torch.equal(a, b) for a, b in zip(dpm.sample_unipc_requests(xs, steps=7), want))
    plan = H._plan(dpm, ns, 7, 2, "bh2")
    res = C.c_int(-1)
    rb, keep = _run_buffers(xs[0], E, plan, dt)
    L.check(L.lib.dpm_plan_run(plan.handle, C.byref(rb), None, None, _stream(), C.byref(res)))
    torch.cuda.synchronize()
    assert torch.equal(keep[res.value], want[0])
    rbs, keeps, results = (L.RunBuffers * 3)(), [], (C.c_int * 3)()
    for r in range(3):
        rbs[r], k = _run_buffers(xs[r], E, plan, dt)
        keeps.append(k)
    L.check(L.lib.dpm_plan_run_multi(plan.handle, rbs, 3, _stream(), None, results))
    torch.cuda.synchronize()
    for r in range(3):
        assert torch.equal(keeps[r][results[r]], want[r]), r
