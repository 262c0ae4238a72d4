"""UniPC stages in the heterogeneous fused launch (stage_kernel_het_unipc) and UniPC requests in the request pool, on the
MI355X.  Kernel level, through the C ABI: dpm_stage_launch_multi with per_request_stages = 1 on mixes of all four UniPC
sub-shapes with first- and second-order records must give every request the bits of its own dpm_stage_launch AND of the fp32
numpy double of the stage (tests/unipc_double.py), and must really be one launch per 16 requests.  End to end:
RequestPool.submit_unipc against sample_unipc, bit for bit.  Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import kernel_double as KD
import unipc_double as UD
from dpm_solver_amd import _lib as L
from test_gpu_unipc import PAIRS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_DT = {torch.float32: L.DTYPE_F32, torch.float16: L.DTYPE_F16, torch.bfloat16: L.DTYPE_BF16}
N = 4 * 4 * 32 * 32                 # 16384 elements: 8 tiles, more than one super-tile per request
N_RAGGED = N + 2048 + 8             # a last tile of one 8-element group
SHAPES = [(False, False), (False, True), (True, False), (True, True)]      # (second-order corrector, second-order predictor)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    yield
    torch.cuda.synchronize()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _stage(form, dp=False, p2=False, guidance="uncond", model="noise", index=3, alpha=0.8, seed=0):
    """a stage record with scalars of realistic magnitude: DPM_FORM_UNIPC with its two sub-shape flags, or a first-order /
    second-order / third-order multistep record of the same (data-prediction) plan family"""
    r = np.random.default_rng(seed + 17)
    st = L.Stage()
    st.index, st.form, st.model_type, st.guidance = index, form, L.MODEL[model], L.GUIDE[guidance]
    st.flags = L.F_TO_X0 | L.F_STORE_M
    if form == L.FORM_UNIPC:
        st.flags |= (L.F_UNIPC_DP if dp else 0) | (L.F_UNIPC_P2 if p2 else 0)
    st.emits_state = 1
    st.alpha_e, st.sigma_e = alpha, float(np.sqrt(1 - alpha * alpha))
    st.cfg_scale = 2.5
    st.cx, st.c0, st.c1, st.c2 = 0.83 + 0.01 * r.random(), -0.47 - 0.01 * r.random(), -0.238, -0.208
    st.k[0], st.k[1], st.k[2], st.k[3] = 0.6685, -0.2782, -0.6686, 0.31
    return st


def _mix(n_req, guidance="uncond", model="noise", alpha=0.8):
    """request r: the four UniPC sub-shapes, a first-order and a second-order record, in turn"""
    sts = []
    for r in range(n_req):
        k = r % 6
        if k < 4:
            sts.append(_stage(L.FORM_UNIPC, *SHAPES[k], guidance=guidance, model=model, index=1 + r % 5, alpha=alpha, seed=r))
        else:
            sts.append(_stage(L.FORM_LIN1 if k == 4 else L.FORM_TWO, guidance=guidance, model=model, index=r % 5, alpha=alpha,
                              seed=r))
    return sts


class Case:
    """the operands of one request as CPU tensors (for the double) and, cloned, on the GPU (for the kernels)"""

    def __init__(self, st, n, sdt, edt, batch=4, offset=0, xc=False, stride=False, sep_xe=False, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.st, self.n, self.batch, self.sdt, self.edt = st, n, batch, sdt, edt
        cfg = st.guidance == L.GUIDE["classifier-free"]
        mk = lambda dt, m=n: torch.randn(m + offset, generator=g).to(dt)
        out = lambda: torch.zeros(n + offset).to(sdt)
        per = n // batch
        self.t = dict(x=mk(sdt), xe=mk(sdt) if sep_xe else None, h1=mk(sdt), h2=mk(sdt),
                      e0=mk(edt, 2 * n if stride else n), e1=(mk(edt, 2 * n if stride else n) if cfg else None),
                      x_out=out(), m_out=out(), x_out2=out() if (cfg or xc) else None)
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


def _bits(t):
    return t.cpu().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _launch_multi(cases, devs):
    R = len(cases)
    opts = L.LaunchOpts()
    opts.per_request_stages = 1
    arr, starr = (L.Buffers * R)(), (L.Stage * R)()
    for r, (c, d) in enumerate(zip(cases, devs)):
        arr[r], starr[r] = c.buffers(d, opts if r == 0 else None), c.st
    L.check(L.lib.dpm_stage_launch_multi(starr, arr, R, _stream()))
    torch.cuda.synchronize()


def _check_against_singles_and_double(cases, what):
    """one per-request-stage multi launch; every x_out, m_out, x_out2 against one dpm_stage_launch per request and the double"""
    devs = [c.gpu() for c in cases]
    _launch_multi(cases, devs)
    for r, c in enumerate(cases):
        single = c.gpu()
        L.check(L.lib.dpm_stage_launch(C.byref(c.st), C.byref(c.buffers(single)), _stream()))
        torch.cuda.synchronize()
        want = c.expect()
        for k in ("x_out", "m_out", "x_out2"):
            if want[k] is not None:
                assert torch.equal(_bits(devs[r][k]), _bits(single[k])), (what, r, c.st.form, c.st.flags, k, "single launch")
                assert torch.equal(_bits(devs[r][k]), _bits(want[k])), (what, r, c.st.form, c.st.flags, k, "double")
        assert float(want["x_out"].float().abs().max()) > 0.1
    return devs


@pytest.mark.parametrize("sdt,edt", PAIRS, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("n_req,n", [(2, N), (5, N), (5, N_RAGGED), (16, N), (17, N), (33, N)])
def test_mixed_unipc_records_equal_the_single_launches_and_the_double(sdt, edt, n_req, n):
    for guidance in ("uncond", "classifier-free"):
        for model, alpha in (("noise", 0.8), ("v", 0.6)):          # the compile-time and the generic prologue
            sts = _mix(n_req, guidance, model, alpha)
            cases = [Case(sts[r], n, sdt, edt, seed=r) for r in range(n_req)]
            devs = _check_against_singles_and_double(cases, (sdt, edt, n_req, n, guidance, model))
            if guidance == "classifier-free":
                assert all(torch.equal(d["x_out2"], d["x_out"]) for d in devs)      # the duplicate store


def _stage_kernels(fn):
    """names of the stage kernels fn() launches, one entry per launch.  torch's profiler, as test_gpu_pool.py counts a tick's
    launches: it runs on the product library (fused_first is the lab build's, and only on the lockstep entry point -- the
    per-request-stage path takes no events) and it names the kernel, so a fused launch by another family would show.  It relies
    on the profiler reporting the demangled name, which contains the kernel template's name."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if "stage_kernel" in e.key for _ in range(e.count)]


@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("n_req,launches", [(5, 1), (16, 1), (17, 2), (33, 3)])
def test_unipc_records_are_fused_in_groups_of_16(sdt, n_req, launches):
    """kernels counted, not bits: a mix of UniPC, first-order and second-order records is ONE stage_kernel_het_unipc launch per
    16 requests (a last group of one request is that request's single launch)"""
    sts = _mix(n_req)
    cases = [Case(sts[r], N, sdt, sdt, seed=r) for r in range(n_req)]
    devs = [c.gpu() for c in cases]
    _launch_multi(cases, devs)                    # (first-launch costs outside the profile)
    names = _stage_kernels(lambda: _launch_multi(cases, devs))
    assert len(names) == launches, names
    assert sum("stage_kernel_het_unipc" in n for n in names) == (n_req + 14) // 16, names


def test_requests_the_fused_kernel_does_not_take_fall_back_in_the_same_call():
    sdt = torch.float16
    for dp, p2 in SHAPES:
        mk = lambda seed, **kw: Case(_stage(L.FORM_UNIPC, dp, p2, seed=seed), N, sdt, sdt, seed=seed, **kw)
        cases = [mk(0), mk(1, offset=1), mk(2, xc=True), mk(3), mk(4, sep_xe=True), mk(5, stride=True),
                 Case(_stage(L.FORM_TWO, seed=6), N, sdt, sdt, seed=6), mk(7)]
        _check_against_singles_and_double(cases, ("unfusable", dp, p2))
    cases = [Case(_mix(8)[r], N, sdt, sdt, seed=r, offset=(1 if r in (0, 5) else 0)) for r in range(8)]
    devs = [c.gpu() for c in cases]
    _launch_multi(cases, devs)
    names = _stage_kernels(lambda: _launch_multi(cases, devs))
    assert len(names) == 3 and sum("stage_kernel_het_unipc" in n for n in names) == 1, names


@pytest.mark.parametrize("sdt,edt", [(torch.float16, torch.float16), (torch.float32, torch.float32)],
                         ids=lambda d: str(d).split(".")[-1])
def test_third_order_and_unipc_records_in_one_call(sdt, edt):
    """MS3 and UNIPC never share a group: the first of the two kinds to join a group decides which of them it takes, the
    other kind's records form the next group -- and every request gets its bits"""
    forms = [L.FORM_MS3, L.FORM_UNIPC, L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3, L.FORM_UNIPC, L.FORM_UNIPC]
    for order in (forms, forms[::-1]):
        sts = [_stage(f, r % 2 == 0, r % 3 == 0, index=2 + r, seed=r) for r, f in enumerate(order)]
        cases = [Case(sts[r], N, sdt, edt, seed=r) for r in range(len(sts))]
        devs = _check_against_singles_and_double(cases, ("ms3 + unipc", sdt, order is forms))
        names = _stage_kernels(lambda: _launch_multi(cases, devs))
        assert len(names) == 2 and sum("stage_kernel_het_unipc" in n for n in names) == 1, names


# ---- the pool ---------------------------------------------------------------------------------------------------------
SHAPE = (4, 4, 32, 32)


def _solver(cfg, continuous):
    if continuous:
        ns = D.NoiseScheduleVP("linear")         # (a half state stays half on a continuous schedule with a noise network)
    else:
        betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
        ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    if cfg:
        c = torch.ones(SHAPE[0], device=DEV)
        net = lambda x, t, cond: (0.5 * x.float() + 0.1 * torch.sin(x.float()) * cond.reshape(-1, 1, 1, 1)[:x.shape[0]]).to(x.dtype)
        fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=3.0, condition=c,
                             unconditional_condition=c * 0)
    else:
        fn = D.model_wrapper(lambda x, t: (0.5 * x.float() + 0.1 * torch.sin(x.float())).to(x.dtype), ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")


UNIPC_KW = [dict(steps=8), dict(steps=2, order=2), dict(steps=6, order=1, variant="bh1"), dict(steps=7, skip_type="logSNR"),
            dict(steps=1, order=1), dict(steps=9, variant="bh1", lower_order_final=False)]


def _run(pool, submits, ticks):
    """submits[j](pool) at tick ticks[j]; {j: result}"""
    handles, got, tick = {}, {}, 0
    while tick <= max(ticks) or pool:
        for j, t in enumerate(ticks):
            if t == tick:
                handles[submits[j](pool)] = j
        for h, out in pool.step().items():
            got[handles[h]] = out
        tick += 1
    return got


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_staggered_pool_of_unipc_requests_equals_sample_unipc(dtype, cfg):
    dpm = _solver(cfg, continuous=dtype is torch.float16)
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [torch.randn(SHAPE, generator=g, device=DEV).to(dtype) for _ in UNIPC_KW]
    got = _run(dpm.request_pool(), [lambda p, x=x, kw=kw: p.submit_unipc(x, **kw) for x, kw in zip(xs, UNIPC_KW)],
               [0, 0, 1, 2, 2, 4])
    assert sorted(got) == list(range(len(xs)))
    for j, (x, kw) in enumerate(zip(xs, UNIPC_KW)):
        want = dpm.sample_unipc(x, **kw)
        assert got[j].dtype == want.dtype == dtype and torch.equal(got[j], want), (j, kw)


def test_pool_mixing_unipc_2m_and_sde_requests():
    dpm = _solver(False, continuous=False)
    g = torch.Generator(device=DEV).manual_seed(6)
    xs = [torch.randn(SHAPE, generator=g, device=DEV) for _ in range(6)]
    calls = [("unipc", dict(steps=7)), ("ode", dict(steps=6, order=2)), ("sde", dict(steps=5, seed=0xDEADBEEF12345)),
             ("unipc", dict(steps=5, variant="bh1")), ("ode", dict(steps=8, order=2)), ("sde", dict(steps=6, seed=3))]
    submit = {"unipc": lambda p, x, kw: p.submit_unipc(x, **kw), "ode": lambda p, x, kw: p.submit(x, **kw),
              "sde": lambda p, x, kw: p.submit(x, sde=True, **kw)}
    single = {"unipc": dpm.sample_unipc, "ode": dpm.sample, "sde": dpm.sample_sde}
    got = _run(dpm.request_pool(), [lambda p, x=x, k=k, kw=kw: submit[k](p, x, kw) for x, (k, kw) in zip(xs, calls)],
               [0, 0, 1, 2, 3, 3])
    for j, (x, (k, kw)) in enumerate(zip(xs, calls)):
        assert torch.equal(got[j], single[k](x, **kw)), (j, k, kw)


def test_staggered_unipc_ticks_are_one_launch():
    """16 UniPC-2 requests at 16 different positions -- a stage-0 request, a stage-1 request, steady ones -- and a 2M request's
    worth of second-order records among them: every tick is one stage_kernel_het_unipc launch"""
    dpm = _solver(False, continuous=True)
    g = torch.Generator(device=DEV).manual_seed(2)
    pool = dpm.request_pool()
    for j in range(15):                   # one admission per tick
        x = torch.randn(SHAPE, generator=g, device=DEV).half()
        if j == 7:
            pool.submit(x, steps=40, order=2)
        else:
            pool.submit_unipc(x, steps=20)
        pool.step()
    names = []
    for _ in range(3):                    # a newcomer at stage 0 in every profiled tick; the oldest is at stage 15 of 20
        pool.submit_unipc(torch.randn(SHAPE, generator=g, device=DEV).half(), steps=1, order=1)
        assert len(pool) == 16
        names += [_stage_kernels(pool.step)]
    assert all(len(n) == 1 and "stage_kernel_het_unipc" in n[0] for n in names), names
