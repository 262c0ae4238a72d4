"""SDE requests in flight together, without a GPU: DPM_Solver.sample_sde_requests and RequestPool.submit(sde=True) on the numpy
doubles -- kernel_double.py (the update), sde_double.py (the noise stage, the seed read from each request's own dpm_launch_opts)
and test_request_pool.py's double of dpm_stage_launch_multi (per-request stage records), composed.  Every result must equal
the request's own sample_sde / sample call bit for bit, and no seed may outlive a call in the solver or in a cache."""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import sde_double as SD
import test_request_pool as TRP
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule

CALLS = TRP.CALLS


@pytest.fixture(autouse=True)
def doubles(monkeypatch):
    SD.install_sde_double(monkeypatch, S, D)
    # the per-request double advances request r by launch_raw_double: give it the noise-aware one (ODE stages pass through)
    monkeypatch.setattr(TRP, "launch_raw_double", SD.launch_raw_noise_double)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", TRP.launch_multi_per_request_double)
    CALLS.clear()


def _solver(cfg=False, continuous=False, **kw):
    ns = D.NoiseScheduleVP("linear") if continuous else make_schedule("sd")
    if cfg:
        def net(x, t, c):
            return torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]).to(x.dtype)
        c = torch.ones(2)
        fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=3.0, condition=c,
                             unconditional_condition=c * 0)
    else:
        def net(x, t):
            return torch.tanh(x * 0.7) + (0.01 * t.reshape(-1, 1, 1, 1)).to(x.dtype)
        fn = D.model_wrapper(net, ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", **kw)


def _xs(R, dtype=torch.float32, shape=(2, 3, 8, 8), seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=g).to(dtype) for _ in range(R)]


SEEDS = [0xDEADBEEF12345, 1, (1 << 64) - 1, 0, 977]


def _seed_in(o):
    return bool(o) and (o.contents.noise_seed_lo != 0 or o.contents.noise_seed_hi != 0)


def _no_seed_left(dpm, seeds):
    assert dpm._noise_seed is None and dpm._group_seeds is None and dpm._group is None
    flat = lambda k: [k] if not isinstance(k, (tuple, list)) else [v for e in k for v in flat(e)]
    big = [s for s in seeds if s > 1 << 20]          # (small seeds collide with shapes and step counts)
    for cache in (dpm._plans, dpm._fast, dpm._fast_groups):
        for key in cache:
            assert not any(type(v) is int and v in big for v in flat(key)), key
    for runs, arrs in dpm._fast_groups.values():
        for a in arrs:
            assert not any(_seed_in(a[r].opts) for r in range(len(runs)))
        for fr in runs:
            assert not any(_seed_in(b.opts) for b in fr.bufs)


@pytest.mark.parametrize("dtz", [False, True], ids=["", "dtz"])
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("solver_type", ["dpmsolver", "taylor"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("R", [2, 5])
def test_requests_equal_their_own_sample_sde(R, order, solver_type, dtype, cfg, dtz):
    dpm = _solver(cfg)
    xs, seeds = _xs(R, dtype), SEEDS[:R]
    kw = dict(steps=6, order=order, solver_type=solver_type, denoise_to_zero=dtz)
    want = [dpm.sample_sde(x, seed=s, **kw) for x, s in zip(xs, seeds)]
    CALLS.clear()
    got = dpm.sample_sde_requests(xs, seeds=seeds, **kw)
    assert len(CALLS) == 6 + dtz and all(c == (R, False) for c in CALLS)      # ONE multi-request call per stage
    assert len(got) == R
    for g, w, x in zip(got, want, xs):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)
        assert g.data_ptr() != x.data_ptr()
    assert not torch.equal(got[0], dpm.sample(xs[0], **kw))                      # (the noise is there)
    _no_seed_left(dpm, seeds)


def test_half_state_with_a_wide_last_stage_runs_request_by_request_with_each_seed():
    # a continuous schedule ends a half-precision denoise_to_zero run in an fp32 stage: the general loop, one request at a time
    dpm = _solver(continuous=True)
    xs, seeds = _xs(3, torch.float16), SEEDS[:3]
    kw = dict(steps=5, denoise_to_zero=True)
    want = [dpm.sample_sde(x, seed=s, **kw) for x, s in zip(xs, seeds)]
    got = dpm.sample_sde_requests(xs, seeds=seeds, **kw)
    assert not CALLS
    assert all(torch.equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
    _no_seed_left(dpm, seeds)


def test_seed_rules():
    dpm = _solver()
    xs = _xs(3)
    kw = dict(steps=5)
    one = lambda x, **k: dpm.sample_sde(x, **kw, **k)
    # explicit seeds; equal seeds on equal x give equal results, distinct seeds distinct ones
    a = dpm.sample_sde_requests([xs[0], xs[0], xs[0], xs[1]], seeds=[5, 6, 5, 5], **kw)
    assert torch.equal(a[0], a[2]) and not torch.equal(a[0], a[1]) and not torch.equal(a[0], a[3])
    assert torch.equal(a[1], one(xs[0], seed=6)) and torch.equal(a[3], one(xs[1], seed=5))
    # seeds=None: one draw per request, in request order, from torch's default generator ...
    torch.manual_seed(11)
    want = [one(x) for x in xs]
    torch.manual_seed(11)
    got = dpm.sample_sde_requests(xs, **kw)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert not torch.equal(got[0], dpm.sample_sde_requests([xs[0], xs[1]], **kw)[0])   # (the generator moved on)
    # ... or from the caller's
    gen = torch.Generator().manual_seed(3)
    want = [one(x, generator=gen) for x in xs]
    got = dpm.sample_sde_requests(xs, generator=torch.Generator().manual_seed(3), **kw)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # tensors and the ends of the range are seeds too
    got = dpm.sample_sde_requests(xs[:2], seeds=[torch.tensor(9), (1 << 64) - 1], **kw)
    assert torch.equal(got[0], one(xs[0], seed=9)) and torch.equal(got[1], one(xs[1], seed=(1 << 64) - 1))
    _no_seed_left(dpm, [])


def test_calls_that_run_request_by_request_keep_each_seed():
    xs, seeds = _xs(3), SEEDS[:3]
    kw = dict(steps=4)
    # a Python corrector on x_t
    dpm = _solver(correcting_xt_fn=lambda x, t, step: x * 0.99)
    want = [dpm.sample_sde(x, seed=s, **kw) for x, s in zip(xs, seeds)]
    got = dpm.sample_sde_requests(xs, seeds=seeds, **kw)
    assert not CALLS and all(torch.equal(g, w) for g, w in zip(got, want))
    dpm = _solver()
    # return_intermediate: a (result, list) pair per request
    got = dpm.sample_sde_requests(xs, seeds=seeds, return_intermediate=True, **kw)
    for (g, gi), x, s in zip(got, xs, seeds):
        w, wi = dpm.sample_sde(x, seed=s, return_intermediate=True, **kw)
        assert torch.equal(g, w) and len(gi) == len(wi) and all(torch.equal(p, q) for p, q in zip(gi, wi))
    # a single request, mixed shapes
    assert torch.equal(dpm.sample_sde_requests(xs[:1], seeds=[4], **kw)[0], dpm.sample_sde(xs[0], seed=4, **kw))
    mixed = [xs[0], xs[1][:1]]
    got = dpm.sample_sde_requests(mixed, seeds=[4, 5], **kw)
    assert torch.equal(got[0], dpm.sample_sde(mixed[0], seed=4, **kw)) and torch.equal(got[1], dpm.sample_sde(mixed[1], seed=5, **kw))
    assert not CALLS
    assert dpm.sample_sde_requests([], **kw) == []
    _no_seed_left(dpm, seeds)


def test_auto_capture_is_bypassed():
    dpm = _solver()
    dpm.auto_capture = 1
    xs = _xs(2)
    for _ in range(3):        # a captured replay would need a device: the calls stay eager, with their seeds
        a = dpm.sample_sde_requests(xs, seeds=[1, 2], steps=4)
    b = dpm.sample_sde_requests(xs, seeds=[2, 1], steps=4)
    assert not dpm._auto and not torch.equal(a[0], b[0])
    assert torch.equal(b[1], dpm.sample_sde(xs[1], seed=1, steps=4))


# (tick of admission, SDE request?, kwargs): different step counts and orders, both solver types, denoise_to_zero, another
# skip type; ODE requests of several methods in between
POOL_MIX = [
    (0, True, dict(steps=8, order=2)),
    (0, False, dict(steps=5, order=3)),
    (1, True, dict(steps=6, order=1)),
    (2, False, dict(steps=6, order=2, method="singlestep", solver_type="taylor")),
    (2, True, dict(steps=7, order=2, solver_type="taylor")),
    (3, True, dict(steps=4, order=2, denoise_to_zero=True)),
    (4, False, dict(steps=8, order=2)),
    (4, True, dict(steps=9, order=2, skip_type="logSNR", lower_order_final=False)),
    (6, True, dict(steps=8, order=2)),
    (9, True, dict(steps=3, order=1, skip_type="time_quadratic")),
]


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("first_is_sde", [True, False])
def test_pool_of_sde_and_ode_requests_staggered(cfg, first_is_sde):
    dpm = _solver(cfg)
    mix = POOL_MIX if first_is_sde else [POOL_MIX[1], POOL_MIX[0]] + POOL_MIX[2:]
    xs = _xs(len(mix))
    seeds = [1000 + 17 * j for j in range(len(mix))]
    want = [dpm.sample_sde(x, seed=s, **kw) if sde else dpm.sample(x, **kw) for x, s, (_, sde, kw) in zip(xs, seeds, mix)]
    CALLS.clear()
    pool = dpm.request_pool()
    handles, got = {}, {}
    tick = 0
    while tick <= max(t for t, _, _ in mix) or pool:
        for j, (t, sde, kw) in enumerate(mix):
            if t == tick:
                handles[pool.submit(xs[j], sde=True, seed=seeds[j], **kw) if sde else pool.submit(xs[j], **kw)] = j
        n_active = len(pool)
        for h, out in pool.step().items():
            got[handles[h]] = out
        if n_active:
            assert CALLS[-1] == (n_active, True)      # ONE multi-request call per tick, with per-request records
        assert pool._opts.noise_seed_lo == 0 and pool._opts.noise_seed_hi == 0
        tick += 1
    assert sorted(got) == list(range(len(mix)))
    for j, w in enumerate(want):
        assert got[j].dtype == w.dtype and torch.equal(got[j], w), mix[j]
    assert dpm._noise_seed is None
    for key, frs in pool._free.items():
        assert not any(s in key for s in seeds)
        assert not any(_seed_in(b.opts) for fr in frs for b in fr.bufs)


def test_pool_seed_is_resolved_at_submission():
    dpm = _solver()
    x = _xs(1)[0]
    pool = dpm.request_pool()
    torch.manual_seed(21)
    h1 = pool.submit(x, steps=4, sde=True)
    h2 = pool.submit(x, steps=4, sde=True, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(99)                 # later draws do not matter
    done = {}
    while pool:
        done.update(pool.step())
    torch.manual_seed(21)
    assert torch.equal(done[h1], dpm.sample_sde(x, steps=4))
    assert torch.equal(done[h2], dpm.sample_sde(x, steps=4, generator=torch.Generator().manual_seed(5)))


def test_pool_scratch_reuse_does_not_leak_a_seed():
    dpm = _solver()
    x1, x2, x3 = _xs(3)
    kw = dict(steps=4, order=2)
    pool = dpm.request_pool()
    done = {}
    h1 = pool.submit(x1, sde=True, seed=SEEDS[0], **kw)
    while pool:
        done.update(pool.step())
    (key, frs), = pool._free.items()
    fr0 = frs[0]
    assert SEEDS[0] not in key and not any(_seed_in(b.opts) for b in fr0.bufs)
    h2 = pool.submit(x2, **kw)                      # an ODE request of the same steps / order / shape: no noise, no seed
    h3 = pool.submit(x3, sde=True, seed=5, **kw)    # an SDE request with another seed on the first one's records
    pool.step()
    assert pool._active[h3].fr is fr0 and pool._active[h2].fr is not fr0
    while pool:
        done.update(pool.step())
    assert torch.equal(done[h1], dpm.sample_sde(x1, seed=SEEDS[0], **kw))
    assert torch.equal(done[h2], dpm.sample(x2, **kw))
    assert torch.equal(done[h3], dpm.sample_sde(x3, seed=5, **kw))
    assert not any(_seed_in(b.opts) for frl in pool._free.values() for fr in frl for b in fr.bufs)


class Reached(Exception):
    """a device entry point was reached"""


def test_errors_come_before_any_device_entry_point(monkeypatch):
    def reached(*a, **k):
        raise Reached()
    for name in ("_launch_stage", "_stage_launch_raw", "_stage_launch_multi_raw", "_launch_ctx", "_require_gpu"):
        monkeypatch.setattr(S, name, reached)
    ns = make_schedule("sd")
    net = lambda x, t: x
    xs = _xs(2)
    many = lambda dpm, *a, **k: dpm.sample_sde_requests(xs, *a, **k)
    pooled = lambda dpm, *a, **k: dpm.request_pool().submit(xs[0], *a, sde=True, **k)

    def same_error(dpm, pool=True, **kw):
        """sample_sde's error, from sample_sde_requests and from the pool: same type, same text"""
        with pytest.raises((NotImplementedError, ValueError, AssertionError)) as one:
            dpm.sample_sde(xs[0], **kw)
        for call in (many, pooled) if pool else (many,):
            with pytest.raises(type(one.value)) as e:
                call(dpm, **kw)
            assert str(e.value) == str(one.value)
        return str(one.value)

    dpm = D.DPM_Solver(net, ns, algorithm_type="dpmsolver++")
    assert "noise-prediction" in same_error(D.DPM_Solver(net, ns, algorithm_type="dpmsolver"))
    assert "thresholding" in same_error(D.DPM_Solver(net, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding"))
    assert "must be 1 or 2" in same_error(dpm, order=3)
    # (the pool asks for a device tensor before it plans, as it does for ODE requests)
    assert "skip_type" in same_error(dpm, pool=False, skip_type="nope")
    assert "solver_type" in same_error(dpm, pool=False, solver_type="nope")
    same_error(dpm, pool=False, steps=1, order=2)
    with pytest.raises(NotImplementedError, match="callable correcting_x0_fn"):
        many(D.DPM_Solver(net, ns, algorithm_type="dpmsolver++", correcting_x0_fn=lambda x0, t: x0))
    with pytest.raises(NotImplementedError, match="sample_sde: double-precision states"):
        dpm.sample_sde_requests([xs[0], xs[1].double()], seeds=[1, 2])
    with pytest.raises(NotImplementedError, match="sample_sde: double-precision states"):
        dpm.request_pool().submit(xs[0].double(), sde=True, seed=1)
    with pytest.raises(ValueError, match="not both"):
        many(dpm, seeds=[1, 2], generator=torch.Generator())
    with pytest.raises(ValueError, match="3 seeds for 2 requests"):
        many(dpm, seeds=[1, 2, 3])
    for bad in (-1, 1 << 64, 1.5, True):
        with pytest.raises(ValueError, match="sample_sde: `seed` must be"):
            many(dpm, seeds=[1, bad])
        with pytest.raises(ValueError, match="sample_sde: `seed` must be"):
            pooled(dpm, seed=bad)
    pool = dpm.request_pool()
    with pytest.raises(ValueError, match="not both"):
        pool.submit(xs[0], sde=True, seed=1, generator=torch.Generator())
    with pytest.raises(ValueError, match="belong to an SDE request"):
        pool.submit(xs[0], seed=1)
    with pytest.raises(ValueError, match="belong to an SDE request"):
        pool.submit(xs[0], generator=torch.Generator())
    for method in ("singlestep", "singlestep_fixed", "adaptive"):
        with pytest.raises(ValueError, match="method='multistep'"):
            pool.submit(xs[0], sde=True, seed=1, method=method)
    assert not pool
    with pytest.raises(Reached):          # ... and when the checks pass, the device is what comes next
        many(dpm, seeds=[1, 2])
    with pytest.raises(Reached):
        pooled(dpm, seed=1)
