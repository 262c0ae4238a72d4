"""DPM_Solver.request_pool (continuous batching) on CPU: the HIP kernels replaced by the numpy double (tests/kernel_double.py),
plus a double of dpm_stage_launch_multi that honours dpm_launch_opts.per_request_stages.  Pool results must equal sample()
of every request bit for bit, whatever else was in flight."""
import ctypes as C_

import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule
from kernel_double import _Ref, install_cpu_double, launch_raw_double

CALLS = []


def launch_multi_per_request_double(st, bufs, n_req, stream):
    """dpm_stage_launch_multi: with bs[0].opts->per_request_stages == 1, request r is advanced by st[r]"""
    per = bool(bufs[0].opts) and bufs[0].opts.contents.per_request_stages == 1
    CALLS.append((int(n_req), per))
    for r in range(int(n_req)):
        rc = launch_raw_double(_Ref(st[r] if per else st._obj), _Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


@pytest.fixture(autouse=True)
def cpu_double(monkeypatch):
    install_cpu_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_per_request_double)
    CALLS.clear()


def _solver(algorithm_type, cfg, model_type="noise"):
    ns = make_schedule("sd")
    if cfg:
        def net(x, t, c):
            return torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]])
        c = torch.ones(2)
        fn = D.model_wrapper(net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=c, unconditional_condition=c * 0)
    else:
        def net(x, t):
            return torch.tanh(x * 0.7) + 0.01 * t.reshape(-1, 1, 1, 1)
        fn = D.model_wrapper(net, ns, model_type=model_type)
    return D.DPM_Solver(fn, ns, algorithm_type=algorithm_type)


# (tick of admission, sample() kwargs): steps below 10 (lower_order_final changes the last forms), orders 1-3, every
# method of a stage plan, both solver types, denoise_to_zero, another skip type
MIX = [
    (0, dict(steps=8, order=2)),
    (0, dict(steps=5, order=3)),
    (1, dict(steps=6, order=1)),
    (2, dict(steps=9, order=3, method="singlestep")),
    (2, dict(steps=6, order=2, method="singlestep", solver_type="taylor")),
    (3, dict(steps=7, order=2, method="singlestep_fixed")),
    (4, dict(steps=12, order=3, skip_type="logSNR", lower_order_final=False)),
    (4, dict(steps=4, order=2, denoise_to_zero=True, solver_type="taylor")),
    (5, dict(steps=10, order=2)),
    (9, dict(steps=3, order=3, method="singlestep", skip_type="time_quadratic")),
]


@pytest.mark.parametrize("algorithm_type", ["dpmsolver", "dpmsolver++"])
@pytest.mark.parametrize("cfg", [False, True])
def test_pool_equals_sample_staggered(algorithm_type, cfg):
    dpm = _solver(algorithm_type, cfg)
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(2, 3, 8, 8, generator=g) for _ in MIX]
    want = [dpm.sample(x, **kw) for x, (_, kw) in zip(xs, MIX)]
    CALLS.clear()
    pool = dpm.request_pool()
    handles, got = {}, {}
    tick = 0
    while tick <= max(t for t, _ in MIX) or pool:
        for j, (t, kw) in enumerate(MIX):
            if t == tick:
                handles[pool.submit(xs[j], **kw)] = j
        n_active = len(pool)
        for h, out in pool.step().items():
            got[handles[h]] = out
        if n_active:
            assert CALLS[-1] == (n_active, True)      # ONE multi-request call per tick, with per-request records
        tick += 1
    assert sorted(got) == list(range(len(MIX)))
    for j, w in enumerate(want):
        assert got[j].dtype == w.dtype and torch.equal(got[j], w), MIX[j]
        assert got[j].data_ptr() != xs[j].data_ptr()


def test_pool_reuses_scratch_and_hands_out_fresh_results():
    dpm = _solver("dpmsolver++", False)
    g = torch.Generator().manual_seed(1)
    x1, x2 = torch.randn(2, 3, 8, 8, generator=g), torch.randn(2, 3, 8, 8, generator=g)
    pool = dpm.request_pool()
    h1 = pool.submit(x1, steps=4, order=2)
    done = {}
    while pool:
        done.update(pool.step())
    fr = pool._free and next(iter(pool._free.values()))[0]
    h2 = pool.submit(x2, steps=4, order=2)
    pool.step()
    assert pool._active[h2].fr is fr                 # the finished request's launch records and scratch
    while pool:
        done.update(pool.step())
    assert torch.equal(done[h1], dpm.sample(x1, steps=4, order=2))
    assert torch.equal(done[h2], dpm.sample(x2, steps=4, order=2))
    assert done[h1].data_ptr() != done[h2].data_ptr()


def test_pool_no_fuse_and_other_model_types():
    """x_start / v networks (the generic prologue) and a solver whose options travel in bs[0].opts"""
    for mt in ("x_start", "v"):
        dpm = _solver("dpmsolver++", False, model_type=mt)
        dpm.thr_spin_limit = 7                        # the solver's own launch options are kept next to the flag
        x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(5))
        pool = dpm.request_pool()
        h = pool.submit(x, steps=5, order=3)
        out = {}
        while pool:
            out.update(pool.step())
        assert torch.equal(out[h], dpm.sample(x, steps=5, order=3))


def test_submit_refuses_unsupported_options():
    dpm = _solver("dpmsolver++", False)
    x = torch.randn(2, 3, 8, 8)
    pool = dpm.request_pool()
    with pytest.raises(NotImplementedError, match="adaptive"):
        pool.submit(x, method="adaptive")
    with pytest.raises(NotImplementedError, match="return_intermediate"):
        pool.submit(x, return_intermediate=True)
    with pytest.raises(ValueError, match="wrong method"):
        pool.submit(x, method="bogus")
    # sample()'s own argument errors
    with pytest.raises(ValueError, match="skip_type"):
        pool.submit(x, skip_type="nope")
    with pytest.raises(ValueError, match="'order' must be"):
        pool.submit(x, order=4, method="singlestep")
    with pytest.raises(AssertionError):
        pool.submit(x, steps=2, order=3)
    pool.submit(x, steps=4)
    with pytest.raises(ValueError, match="shape"):
        pool.submit(torch.randn(1, 3, 8, 8))
    with pytest.raises(ValueError, match="dtype"):
        pool.submit(x.double())
    with pytest.raises(ValueError, match="at least one dimension"):
        dpm.request_pool().submit(torch.randn(()))
    cxt = D.DPM_Solver(dpm.model, dpm.noise_schedule, correcting_xt_fn=lambda x, t, s: x)
    with pytest.raises(NotImplementedError, match="correcting_xt_fn"):
        cxt.request_pool().submit(x)
    cx0 = D.DPM_Solver(dpm.model, dpm.noise_schedule, correcting_x0_fn=lambda x0, t: x0)
    with pytest.raises(NotImplementedError, match="correcting_x0_fn"):
        cx0.request_pool().submit(x)


def test_launch_opts_field():
    assert C_.sizeof(L.LaunchOpts) == 32
    assert L.lib.dpm_sizeof(5) == 32                  # DPM_SIZEOF_LAUNCH_OPTS
    assert L.LaunchOpts.per_request_stages.offset == 12
    assert L.lib.dpm_version() >= 202
