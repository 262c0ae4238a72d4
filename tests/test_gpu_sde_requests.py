"""GPU tests of the fused SDE stages (DPM_F_NOISE in dpm_stage_launch_multi, lockstep and per-request stages): every request of
a fused launch must end bit-identical to its own dpm_stage_launch with its own dpm_launch_opts -- new state, stored model value
and duplicate store -- for every dtype pair, both forms, both guidance kinds, both prologues, request counts around
DPM_MULTI_MAX, a size with the XCD remap and two tiles per super-tile, and a request without options (seed 0).  Then
dpm_plan_run_multi, DPM_Solver.sample_sde_requests and the request pool against sample_sde.  Run on an MI355X:  pytest -m gpu
"""
import ctypes as C_
import random

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
from dpm_solver_amd import _lib as L
from test_gpu_het import PAIRS, Req, _stage, check
from test_gpu_multi import make_requests, sd_schedule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = (256, 4, 64, 64)       # 2048 tiles per request: XCD-contiguous remap (2-byte states), two tiles per super-tile (4-byte)
SMALL = (2, 4, 24, 32)       # 3 tiles


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    yield
    torch.cuda.synchronize()


def _opts(seed, **kw):
    o = L.LaunchOpts()
    o.noise_seed_lo, o.noise_seed_hi = seed & 0xffffffff, seed >> 32
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _noise_stage(rng, form, index, model_type="noise", cfg=False, to_x0=True, store_m=True):
    st = _stage(rng, form, L.MODEL[model_type], L.GUIDE["classifier-free"] if cfg else L.GUIDE["uncond"], to_x0, store_m)
    st.flags = (st.flags & ~L.F_BASE_HIST) | L.F_NOISE
    st.index = index
    return st


def _seeds(rng, n_req):
    """a seed per request; request 1 (or the only one besides 0) has no dpm_launch_opts at all: seed 0"""
    return [None if r == 1 else rng.getrandbits(64) for r in range(n_req)]


def lockstep_both(st, reqs, seeds, **opt_kw):
    """(one dpm_stage_launch_multi, one dpm_stage_launch per request with that request's options): their outputs"""
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    R = len(reqs)
    outs_m, outs_s = [q.outputs() for q in reqs], [q.outputs() for q in reqs]
    opts = [None if s is None else _opts(s, **opt_kw) for s in seeds]
    arr_b = (L.Buffers * R)(*[q.buffers(o) for q, o in zip(reqs, outs_m)])
    for r in range(R):
        if opts[r] is not None:
            arr_b[r].opts = C_.pointer(opts[r])
    L.check(L.lib.dpm_stage_launch_multi(C_.byref(st), arr_b, R, stream))
    torch.cuda.synchronize()
    for r, q in enumerate(reqs):
        b = q.buffers(outs_s[r])
        if opts[r] is not None:
            b.opts = C_.pointer(opts[r])
        L.check(L.lib.dpm_stage_launch(C_.byref(st), C_.byref(b), stream))
    torch.cuda.synchronize()
    return outs_m, outs_s


def _lockstep_case(sd, ed, form, cfg, model_type, to_x0, n_req, shape, seed, **opt_kw):
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    st = _noise_stage(rng, form, index=rng.randrange(0, 50), model_type=model_type, cfg=cfg, to_x0=to_x0)
    reqs = [Req(g, shape, sd, ed, cfg) for _ in range(n_req)]
    seeds = _seeds(rng, n_req)
    outs_m, outs_s = lockstep_both(st, reqs, seeds, **opt_kw)
    check([st] * n_req, reqs, outs_m, outs_s)
    # the requests differ in their noise: request 1 (seed 0) and request 0 on the SAME operands would otherwise be equal
    assert not torch.equal(outs_m[0]["x"], outs_m[1]["x"])
    return st, reqs, seeds, outs_m


@pytest.mark.parametrize("sd,ed", PAIRS)
@pytest.mark.parametrize("form", [L.FORM_LIN1, L.FORM_TWO])
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("model_type,to_x0", [("noise", True), ("v", True)], ids=["x0", "generic"])
def test_lockstep_equals_single(sd, ed, form, cfg, model_type, to_x0):
    """every kernel of the family (dtype pair x form x guidance x prologue), one group and a full group plus a remainder"""
    for n_req in (5, 33):
        _lockstep_case(sd, ed, form, cfg, model_type, to_x0, n_req, SMALL, seed=100 * n_req + form + 2 * cfg)


@pytest.mark.parametrize("n_req", [2, 5, 16, 32, 33, 40])
@pytest.mark.parametrize("sd,ed", [(torch.float16, torch.float16), (torch.float32, torch.float32)])
def test_lockstep_request_counts(sd, ed, n_req):
    _lockstep_case(sd, ed, L.FORM_TWO, False, "noise", True, n_req, SMALL, seed=n_req)


@pytest.mark.parametrize("sd,ed", PAIRS)
@pytest.mark.parametrize("n_req,form,cfg,model_type", [(2, L.FORM_TWO, False, "noise"), (5, L.FORM_LIN1, True, "noise"),
                                                       (33, L.FORM_TWO, False, "noise"), (3, L.FORM_TWO, True, "x_start")])
def test_lockstep_at_request_size(sd, ed, n_req, form, cfg, model_type):
    """[256,4,64,64] requests: the XCD-contiguous tile mapping of 2-byte states and two tiles per super-tile of 4-byte ones
    (the split layout's element index) give the element index of the single launch"""
    if n_req == 33 and (sd, ed) not in ((torch.float16, torch.float16), (torch.float32, torch.float32)):
        n_req = 4
    _lockstep_case(sd, ed, form, cfg, model_type, True, n_req, BIG, seed=7 * n_req)


def test_lockstep_noise_depends_on_seed_stage_and_element_only():
    """the same operands in two requests with the same seed give the same bits whatever their place in the launch; another
    seed or another stage index does not"""
    rng = random.Random(5)
    g = torch.Generator().manual_seed(5)
    q = Req(g, BIG, torch.float16, torch.float16, False)
    st = _noise_stage(rng, L.FORM_TWO, index=3)
    reqs = [q] * 6
    outs_m, outs_s = lockstep_both(st, reqs, [11, None, 11, 12, 11, 0])
    check([st] * 6, reqs, outs_m, outs_s)
    x = [o["x"] for o in outs_m]
    assert torch.equal(x[0], x[2]) and torch.equal(x[0], x[4]) and torch.equal(x[1], x[5]) and not torch.equal(x[0], x[3])
    st.index = 4
    again, _ = lockstep_both(st, reqs[:2], [11, None])
    assert not torch.equal(again[0]["x"], x[0])


def test_lockstep_no_fuse_and_unfused_shapes():
    """no_fuse, a ragged size and unaligned views run request by request (stage_kernel_scalar_noise): the same bits"""
    _lockstep_case(torch.float16, torch.float16, L.FORM_TWO, False, "noise", True, 5, SMALL, seed=1, no_fuse=1)
    _lockstep_case(torch.float32, torch.float32, L.FORM_TWO, True, "noise", True, 4, (3, 5, 7), seed=2)
    rng = random.Random(3)
    g = torch.Generator().manual_seed(3)
    st = _noise_stage(rng, L.FORM_LIN1, index=9)
    reqs = [Req(g, SMALL, torch.float16, torch.float16, False, offset=(1 if r == 2 else 0)) for r in range(4)]
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs_m, outs_s = [q.outputs(1 if r == 2 else 0) for r, q in enumerate(reqs)], [q.outputs(1 if r == 2 else 0) for r, q in enumerate(reqs)]
    opts = [_opts(50 + r) for r in range(4)]
    arr_b = (L.Buffers * 4)(*[q.buffers(o) for q, o in zip(reqs, outs_m)])
    for r in range(4):
        arr_b[r].opts = C_.pointer(opts[r])
    L.check(L.lib.dpm_stage_launch_multi(C_.byref(st), arr_b, 4, stream))
    for r, q in enumerate(reqs):
        b = q.buffers(outs_s[r])
        b.opts = C_.pointer(opts[r])
        L.check(L.lib.dpm_stage_launch(C_.byref(st), C_.byref(b), stream))
    torch.cuda.synchronize()
    check([st] * 4, reqs, outs_m, outs_s)


def test_lockstep_validity_errors_are_the_single_launch_s():
    rng = random.Random(1)
    g = torch.Generator().manual_seed(1)
    st = _noise_stage(rng, L.FORM_MS3, index=2)
    reqs = [Req(g, SMALL, torch.float16, torch.float16, False) for _ in range(3)]
    outs = [q.outputs() for q in reqs]
    arr_b = (L.Buffers * 3)(*[q.buffers(o) for q, o in zip(reqs, outs)])
    rc = L.lib.dpm_stage_launch_multi(C_.byref(st), arr_b, 3, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and b"DPM_F_NOISE is valid on LIN1 / TWO stages only" in L.lib.dpm_last_error()
    assert all(torch.isnan(o["x"].float()).all() for o in outs)


# ---- per-request stages -------------------------------------------------------------------------
def het_both(sts, reqs, offsets, seeds, no_fuse=False):
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    R = len(reqs)
    outs_m = [q.outputs(o) for q, o in zip(reqs, offsets)]
    outs_s = [q.outputs(o) for q, o in zip(reqs, offsets)]
    opts = [None if s is None else _opts(s) for s in seeds]
    if opts[0] is None:
        opts[0] = _opts(0)
    opts[0].per_request_stages = 1
    opts[0].no_fuse = 1 if no_fuse else 0
    arr_st = (L.Stage * R)(*sts)
    arr_b = (L.Buffers * R)(*[q.buffers(o) for q, o in zip(reqs, outs_m)])
    for r in range(R):
        if opts[r] is not None:
            arr_b[r].opts = C_.pointer(opts[r])
    L.check(L.lib.dpm_stage_launch_multi(arr_st, arr_b, R, stream))
    torch.cuda.synchronize()
    single = [None if o is None else _opts(int(o.noise_seed_lo) | (int(o.noise_seed_hi) << 32)) for o in opts]
    for r, q in enumerate(reqs):
        b = q.buffers(outs_s[r])
        if single[r] is not None:
            b.opts = C_.pointer(single[r])
        L.check(L.lib.dpm_stage_launch(C_.byref(sts[r]), C_.byref(b), stream))
    torch.cuda.synchronize()
    return outs_m, outs_s


def _het_mix(n_req, sd, ed, seed, cfg=False, model_type="noise", to_x0=True, ode_every=0, odd=False, shape=SMALL):
    """requests at different stage indices with their own scale c2; every `ode_every`-th one an ODE request (any fused form);
    `odd`: one ragged and one unaligned request among them"""
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    sts, reqs, offsets, seeds = [], [], [], []
    for r in range(n_req):
        ode = ode_every and r % ode_every == 1
        if ode:
            st = _stage(rng, rng.choice([L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3]), L.MODEL[model_type],
                        L.GUIDE["classifier-free"] if cfg else L.GUIDE["uncond"], to_x0, rng.random() < 0.6)
        else:
            st = _noise_stage(rng, rng.choice([L.FORM_LIN1, L.FORM_TWO]), index=rng.randrange(0, 30), model_type=model_type,
                              cfg=cfg, to_x0=to_x0, store_m=rng.random() < 0.6)
        off, shp = 0, shape
        if odd and r == 3:
            shp = (3, 5, 7)
        if odd and r == 6:
            off = 1
        sts.append(st)
        reqs.append(Req(g, shp, sd, ed, cfg, offset=off))
        offsets.append(off)
        seeds.append(None if r == 2 else rng.getrandbits(64))
    return sts, reqs, offsets, seeds


@pytest.mark.parametrize("sd,ed", PAIRS)
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("model_type,to_x0", [("noise", True), ("x_start", True)], ids=["x0", "generic"])
def test_het_noise_equals_single(sd, ed, cfg, model_type, to_x0):
    """more than HET_MAX noise requests at different stage indices, ODE requests in between, a ragged and an unaligned one"""
    sts, reqs, offs, seeds = _het_mix(48, sd, ed, seed=31 + 2 * cfg, cfg=cfg, model_type=model_type, to_x0=to_x0, ode_every=4,
                                      odd=True)
    assert sum(1 for st in sts if st.flags & L.F_NOISE) > 2 * 16
    check(sts, reqs, *het_both(sts, reqs, offs, seeds))


@pytest.mark.parametrize("sd,ed", [(torch.float16, torch.float16), (torch.float32, torch.float32), (torch.float32, torch.float16)])
def test_het_noise_at_request_size(sd, ed):
    sts, reqs, offs, seeds = _het_mix(19, sd, ed, seed=9, ode_every=5, shape=BIG)
    check(sts, reqs, *het_both(sts, reqs, offs, seeds))


def test_het_noise_no_fuse():
    sts, reqs, offs, seeds = _het_mix(7, torch.float16, torch.float16, seed=13, ode_every=3)
    check(sts, reqs, *het_both(sts, reqs, offs, seeds, no_fuse=True))


# ---- the native loop and the Python interface -----------------------------------------------------
def test_plan_run_multi_with_per_request_seeds_equals_sample_sde():
    ns = sd_schedule()
    shape, R = (2, 4, 32, 32), 5
    reqs = make_requests(R, shape, torch.float32, torch.float32, seed=21)
    seeds = [4242 + 1000003 * r for r in range(R)]
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: x, ns), ns)
    plan = dpm._get_plan(method="multistep", order=2, steps=10, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1. / ns.total_N, sde=True)
    want = []
    for q, s in zip(reqs, seeds):
        E = q["e0"]
        one = D.DPM_Solver(D.model_wrapper(lambda x, t: E, ns), ns)
        want.append(one.sample_sde(q["x"][0].clone(), steps=10, order=2, seed=s))
    rbs = (L.RunBuffers * R)(*[q["rb"] for q in reqs])
    opts = [_opts(s) for s in seeds]
    for r in range(R):
        rbs[r].opts = C_.pointer(opts[r])
    res = (C_.c_int * R)()
    L.check(L.lib.dpm_plan_run_multi(plan.handle, rbs, R, C_.c_void_p(torch.cuda.current_stream().cuda_stream), None, res))
    torch.cuda.synchronize()
    for r in range(R):
        assert torch.equal(reqs[r]["x"][res[r]], want[r]), r
    assert not torch.equal(want[0], want[1])


def _py_solver(ns, cfg=False, channels_last=False):
    def net(x, t, c=None):
        y = torch.tanh(x * 0.7) * (0.5 if c is None else (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]).to(x.dtype))
        return y.contiguous(memory_format=torch.channels_last) if channels_last else y
    if cfg:
        c = torch.ones(4, device=DEV)
        fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=3.0, condition=c,
                             unconditional_condition=c * 0)
    else:
        fn = D.model_wrapper(net, ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cfg,channels_last", [(False, False), (True, False), (False, True)], ids=["uncond", "cfg", "nhwc"])
def test_sample_sde_requests_and_pool_equal_sample_sde(dtype, cfg, channels_last):
    ns = sd_schedule()
    dpm = _py_solver(ns, cfg, channels_last)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(4, 4, 32, 32, generator=g).to(dtype).to(DEV) for _ in range(5)]
    seeds = [10 ** 15 + 7 * r for r in range(5)]
    kw = dict(steps=8, order=2)
    want = [dpm.sample_sde(x, seed=s, **kw) for x, s in zip(xs, seeds)]
    got = dpm.sample_sde_requests(xs, seeds=seeds, **kw)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.isfinite(a.float()).all() and torch.equal(a, b)
    assert not torch.equal(got[0], dpm.sample_sde_requests(xs, seeds=seeds[::-1], **kw)[0])
    assert all(torch.equal(a, b) for a, b in zip(dpm.sample_sde_requests(xs, seeds=seeds, **kw), want))     # cached records
    # the pool: SDE requests with different step counts, an ODE request in between, staggered
    mix = [(0, True, dict(steps=8, order=2)), (0, False, dict(steps=6, order=3)), (1, True, dict(steps=5, order=1)),
           (3, True, dict(steps=7, order=2, solver_type="taylor")), (3, True, dict(steps=8, order=2))]
    want = [dpm.sample_sde(x, seed=s, **k) if sde else dpm.sample(x, **k) for x, s, (_, sde, k) in zip(xs, seeds, mix)]
    pool = dpm.request_pool()
    handles, done, tick = {}, {}, 0
    while tick <= 3 or pool:
        for j, (t, sde, k) in enumerate(mix):
            if t == tick:
                handles[pool.submit(xs[j], sde=True, seed=seeds[j], **k) if sde else pool.submit(xs[j], **k)] = j
        for h, out in pool.step().items():
            done[handles[h]] = out
        tick += 1
    torch.cuda.synchronize()
    for j, w in enumerate(want):
        assert done[j].dtype == w.dtype and torch.equal(done[j], w), mix[j]


def test_requests_sample_the_right_distribution():
    """test_gpu_sde.py::test_samples_the_right_distribution through sample_sde_requests: 4 requests of [4,4,128,128] with
    distinct seeds, the mean and std of all results together, with that test's tolerance (2 % of s, calibrated there)"""
    ns = D.NoiseScheduleVP("linear")
    mu, s = 0.7, 0.4

    def x0_pred(x, t):
        a = ns.marginal_alpha(t)[:, None, None, None]
        sg = ns.marginal_std(t)[:, None, None, None]
        return mu + a * s * s / (a * a * s * s + sg * sg) * (x - a * mu)
    x_T = torch.randn(16, 4, 128, 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    dpm = D.DPM_Solver(D.model_wrapper(x0_pred, ns, model_type="x_start"), ns)
    ys = dpm.sample_sde_requests(list(x_T.split(4)), seeds=[1, 2, 3, 4], steps=50, order=2, skip_type="logSNR")
    y = torch.cat(ys)
    m, sd = float(y.mean()), float(y.std())
    print("mean %.5f std %.5f" % (m, sd))
    assert abs(m - mu) < 0.02 * s and abs(sd / s - 1) < 0.02, (m, sd)
