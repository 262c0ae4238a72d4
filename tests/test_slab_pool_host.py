"""The slab pool (DPM_Solver.request_pool(slots=S), dpm_solver_amd/slab.py) without a GPU: its host code on the numpy doubles
(tests/table_double.py -- DPM_TABLE_FILL by the real library, the per-request doubles at DPM_TABLE_LAUNCH, plain tensors for
the pinned staging).  A staggered pool of 30 small requests in 24 rows must give every request the bits of its own sample() /
sample_unipc() call, with ONE network call and exactly two multi-request calls (FILL, LAUNCH) per tick; requests that find no
free rows wait and are admitted in order; every refusal comes before any device work."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_double as TD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule

NET_CALLS = []


@pytest.fixture
def doubles(monkeypatch):
    TD.install_table_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _net(x, t, c=None):
    """elementwise in the row: its state, its time and its condition (any number of condition rows that divides x's)"""
    NET_CALLS.append(int(x.shape[0]))
    xf = x.float()
    xc = torch.clamp(xf, -2.0, 2.0)
    out = 0.5 * xf + 0.1 * xc * xc + 0.0001 * t.float().reshape(-1, 1, 1, 1)
    if c is not None:
        out = out * (0.8 + 0.2 * c.float().repeat_interleave(x.shape[0] // c.shape[0], dim=0).reshape(-1, 1, 1, 1))
    return out.to(x.dtype)


def _solver(cfg, dtype, cond=None, uncond=None):
    ns = make_schedule("sd")
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_net, ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", **kw)


def _requests(n=30, seed=208):
    """(tick of submission, kind, kwargs, b): steps 4..9, orders 1..3, 2M-style multistep and UniPC, b in {1, 2, 3}"""
    out = []
    for j in range(n):
        steps, b = 4 + j % 6, 1 + j % 3
        if j % 2:
            kind, kw = "unipc", dict(steps=steps, order=1 + j % 4 // 2, variant=("bh2", "bh1")[j % 3 == 0])
        else:
            kind, kw = "2m", dict(steps=steps, order=1 + (j // 2) % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 0],
                                  denoise_to_zero=(j % 10 == 0))
        out.append((j // 4, kind, kw, b))
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(b, 4, 8, 8, generator=g) for _, _, _, b in out]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, _, b) in enumerate(out)]
    return out, xs, conds


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_slab_pool_equals_every_request_alone(doubles, dtype, cfg):
    reqs, xs, conds = _requests()
    xs = [x.to(dtype) for x in xs]
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=24)
    assert isinstance(pool, SlabPool)
    handles, got, admitted, tick = {}, {}, {}, 0
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kind, kw, b) in enumerate(reqs):
            if t == tick:
                ckw = dict(condition=conds[j][0], unconditional_condition=conds[j][1]) if cfg else {}
                h = (pool.submit_unipc if kind == "unipc" else pool.submit)(xs[j], **kw, **ckw)
                handles[h] = j
        nets, calls = len(NET_CALLS), len(TD.CALLS)
        waiting = [q.h for q in pool._wait]
        done = pool.step()
        for h in waiting:
            if h in pool._rows or h in done:
                admitted.setdefault(h, tick)
        active = len(NET_CALLS) > nets
        if active:
            assert NET_CALLS[nets:] == [48 if cfg else 24]                   # ONE network call per tick, on the whole slab
            R = TD.CALLS[calls][0]
            assert TD.CALLS[calls:] == [(R, L.TABLE_FILL), (R, L.TABLE_LAUNCH)]   # exactly two multi-request calls
        else:
            assert TD.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(reqs)))
    # 30 requests of 60 rows in 24: some waited, and they were admitted in the order they came
    order = [admitted[h] for h in sorted(admitted)]
    assert len(admitted) == len(reqs) and order == sorted(order) and max(order) > max(r[0] for r in reqs)
    # at most one copy per tick beyond the table's: the time vector of a tick that admitted requests
    assert len(TD.COPIES) == pool.copies <= 2 * pool._tick and sum(c == pool._copyb for c in TD.COPIES) == pool._tick
    NET_CALLS.clear()
    for j, (_, kind, kw, b) in enumerate(reqs):
        alone = _solver(cfg, dtype, *[c.expand(b, -1) for c in conds[j]]) if cfg else dpm
        want = (alone.sample_unipc if kind == "unipc" else alone.sample)(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kind, kw)
        assert torch.equal(got[j], want), (j, kind, kw, b)


def test_steady_state_is_one_copy_per_tick(doubles):
    dpm = _solver(False, torch.float32)
    pool = dpm.request_pool(slots=40)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(20)]
    hs = [pool.submit(x, steps=8, order=2) for x in xs]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        done.update(pool.step())
    assert pool.copies == 6 and TD.CALLS[-2:] == [(20, L.TABLE_FILL), (20, L.TABLE_LAUNCH)]
    while pool:
        done.update(pool.step())
    for h, x in zip(hs, xs):
        assert torch.equal(done[h], dpm.sample(x, steps=8, order=2))
    assert pool.step() == {} and not pool


def test_default_conditions_and_waiting_requests(doubles):
    dpm = _solver(True, torch.float32)
    pool = dpm.request_pool(slots=4)
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(3, 4, 8, 8, generator=g) for _ in range(3)]
    hs = [pool.submit(x, steps=5, order=2) for x in xs]           # 9 rows wanted, 4 there: one request at a time
    assert len(pool) == 3
    finished = []
    while pool:
        finished += list(pool.step())
    assert finished == hs
    with pytest.raises(ValueError, match="does not fit 4 slots"):
        pool.submit(torch.randn(5, 4, 8, 8), steps=5)
    with pytest.raises(ValueError, match="does not match the pool's"):
        pool.submit(torch.randn(1, 4, 8, 9), steps=5)
    with pytest.raises(ValueError, match="leading dimension 2 or 1"):
        pool.submit(torch.randn(2, 4, 8, 8), steps=5, condition=torch.ones(3, 1))
    with pytest.raises(ValueError, match="mixed_shapes"):
        dpm.request_pool(slots=4, mixed_shapes=True)
    assert type(dpm.request_pool()).__name__ == "RequestPool"


# ---- refusals: raised on a HOST x, with no double installed -- the device requirement (a RuntimeError) would come first if any
# device work preceded them
def _plain(**kw):
    ns = make_schedule("sd")
    return D.DPM_Solver(D.model_wrapper(_net, ns), ns, algorithm_type="dpmsolver++", **kw)


def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    pool = _plain().request_pool(slots=8)
    for kw, text in ((dict(method="singlestep"), "singlestep or adaptive"), (dict(method="singlestep_fixed"), "singlestep or"),
                     (dict(method="adaptive"), "singlestep or adaptive"), (dict(sde=True), "sde=True"),
                     (dict(return_intermediate=True), "return_intermediate")):
        with pytest.raises(NotImplementedError, match=text):
            pool.submit(x, steps=6, **kw)
    with pytest.raises(NotImplementedError, match="return_intermediate"):
        pool.submit_unipc(x, steps=6, return_intermediate=True)
    ns = make_schedule("sd")
    solvers = {
        "dynamic_thresholding": _plain(correcting_x0_fn="dynamic_thresholding"),
        "correcting_x0_fn / correcting_xt_fn": _plain(correcting_x0_fn=lambda x0, t: x0),
        "correcting_x0_fn / correcting_xt_fn ": _plain(correcting_xt_fn=lambda xt, t, step: xt),
        "classifier guidance": D.DPM_Solver(D.model_wrapper(_net, ns, guidance_type="classifier", condition=torch.ones(1),
                                                            classifier_fn=lambda x, t, c: x.sum()), ns,
                                            algorithm_type="dpmsolver++"),
    }
    for text, dpm in solvers.items():
        with pytest.raises(NotImplementedError, match=text.strip()):
            dpm.request_pool(slots=8).submit(x, steps=6)
    with pytest.raises(NotImplementedError, match="double-precision states"):
        pool.submit(x.double(), steps=6)
    lin = D.NoiseScheduleVP("linear")
    half = D.DPM_Solver(D.model_wrapper(_net, lin), lin, algorithm_type="dpmsolver++")
    with pytest.raises(NotImplementedError, match="explicit state_dtype"):
        half.request_pool(slots=8).submit(x.half(), steps=6)
    # sample()'s own errors, in its order, still before the device requirement ...
    with pytest.raises(AssertionError):
        pool.submit(x, steps=1, order=2)
    with pytest.raises(ValueError, match="Unsupported skip_type"):
        pool.submit(x, steps=6, skip_type="nope")
    with pytest.raises(ValueError, match="sample_unipc: 'order' must be 1 or 2"):
        pool.submit_unipc(x, steps=6, order=3)
    # ... which a well-formed request on the host then meets
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
        pool.submit(x, steps=6)
    assert not pool and pool.step() == {}
