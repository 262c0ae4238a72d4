"""An SDE slab pool (DPM_Solver.request_pool(slots=S, sde=True)) without a GPU: its host code on the numpy doubles of
tests/table_sde_double.py -- DPM_TABLE_FILL | DPM_TABLE_NOISE by the real library, the per-row doubles at LAUNCH.  A staggered
pool of 12 rows holds SDE, 2M and UniPC requests of 1..3 samples; rows free up so that a later SDE request lands in
non-adjacent rows, and every result must still be the bits of sample_sde / sample / sample_unipc on the request alone."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_sde_double as TSD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from test_slab_pool_host import NET_CALLS, _net, _plain, _solver

FILL_N, LAUNCH_N = L.TABLE_FILL | L.TABLE_NOISE, L.TABLE_LAUNCH | L.TABLE_NOISE


@pytest.fixture
def doubles(monkeypatch):
    TSD.install_table_sde_double(monkeypatch, S, D)
    NET_CALLS.clear()


# (tick of submission, kind, kwargs, b).  Tick 0 fills rows 0..10; the requests of rows 0 and 3 finish after three ticks, so
# the three samples of request 6 land in rows 0, 3 and 11; requests 7 and 8 find no free rows and wait.
REQS = [
    (0, "2m", dict(steps=3, order=2), 1),
    (0, "sde", dict(steps=9, order=2, seed=0xDEADBEEF12345), 2),
    (0, "unipc", dict(steps=3, order=2), 1),
    (0, "sde", dict(steps=8, order=1, seed=(1 << 64) - 1), 3),
    (0, "2m", dict(steps=7, order=3, skip_type="logSNR"), 2),
    (0, "unipc", dict(steps=6, order=2, variant="bh1"), 2),
    (3, "sde", dict(steps=5, order=2, solver_type="taylor", denoise_to_zero=True, seed=977), 3),
    (3, "sde", dict(steps=4, order=2, seed=0), 1),
    (4, "2m", dict(steps=4, order=2, denoise_to_zero=True), 2),
    (5, "sde", dict(steps=6, order=2, skip_type="time_quadratic", seed=5), 2),
]


def _alone(dpm, kind, x, kw):
    return {"sde": dpm.sample_sde, "2m": dpm.sample, "unipc": dpm.sample_unipc}[kind](x, **kw)


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_sde_slab_pool_equals_every_request_alone(doubles, dtype, cfg):
    g = torch.Generator().manual_seed(209)
    xs = [torch.randn(b, 4, 8, 8, generator=g).to(dtype) for _, _, _, b in REQS]
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=12, sde=True)
    assert isinstance(pool, SlabPool)
    handles, got, rows_of, tick = {}, {}, {}, 0
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kind, kw, b) in enumerate(REQS):
            if t == tick:
                sub = pool.submit_unipc if kind == "unipc" else pool.submit
                handles[sub(xs[j], sde=True, **kw) if kind == "sde" else sub(xs[j], **kw)] = j
        nets, calls = len(NET_CALLS), len(TSD.CALLS)
        done = pool.step()
        for h, (rws, _) in pool._rows.items():
            rows_of.setdefault(handles[h], list(rws))
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [24 if cfg else 12]                      # ONE network call per tick, on the whole slab
            R = TSD.CALLS[calls][0]
            assert TSD.CALLS[calls:] == [(R, FILL_N), (R, LAUNCH_N)]            # exactly two multi-request calls, flagged
        else:
            assert TSD.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(REQS)))
    assert rows_of[6] == [0, 3, 11], rows_of                                    # one request, three non-adjacent rows
    assert set(TSD.BASES) == {0, 1, 2}
    assert not pool._ropts                                                       # no request's options outlive it
    NET_CALLS.clear()
    for j, (_, kind, kw, b) in enumerate(REQS):
        want = _alone(dpm, kind, xs[j], kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kind, kw)
        assert torch.equal(got[j], want), (j, kind, kw, b)
    # (the noise is there, and sample k of a request does not get sample 0's)
    assert not torch.equal(got[1], dpm.sample(xs[1], steps=9, order=2))
    twice = torch.cat([xs[7], xs[7]])
    out = dpm.sample_sde(twice, steps=4, order=2, seed=0)
    assert torch.equal(out[:1], got[7]) and not torch.equal(out[1:], got[7])


def test_steady_state_is_one_copy_per_tick_and_the_modes_of_either_pool(doubles):
    dpm = _solver(False, torch.float32)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(1 + j % 2, 4, 8, 8, generator=g) for j in range(12)]
    pool = dpm.request_pool(slots=40, sde=True)
    hs = [pool.submit(x, steps=8, order=2, sde=True, seed=100 + j) for j, x in enumerate(xs)]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        done.update(pool.step())
    assert pool.copies == 6 and TSD.CALLS[-2:] == [(18, FILL_N), (18, LAUNCH_N)]
    assert pool._copyb == len(TSD.FILLED["last"]) - 18 * (L.TABLE_ROW_BYTES + L.TABLE_NOISE_BYTES) + 40 * (
        L.TABLE_ROW_BYTES + L.TABLE_NOISE_BYTES) + 4 * 40                       # staging sized for the noise section
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        assert torch.equal(done[h], dpm.sample_sde(x, steps=8, order=2, seed=100 + j))
    # a plain slab pool keeps modes 1 / 2 and the staging it had
    TSD.CALLS.clear()
    plain = dpm.request_pool(slots=40)
    h = plain.submit(xs[0], steps=4, order=2)
    out = {}
    while plain:
        out.update(plain.step())
    assert set(m for _, m in TSD.CALLS) == {L.TABLE_FILL, L.TABLE_LAUNCH}
    assert plain._tabb == (L.TABLE_HEADER_BYTES + 40 * L.TABLE_ROW_BYTES + 15) // 16 * 16
    assert torch.equal(out[h], dpm.sample(xs[0], steps=4, order=2))


def test_seeds_drawn_at_submission(doubles):
    dpm = _solver(False, torch.float32)
    x = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3))
    pool = dpm.request_pool(slots=8, sde=True)
    torch.manual_seed(41)
    h0 = pool.submit(x, steps=5, sde=True)                                     # torch's default CPU generator, here
    h1 = pool.submit(x, steps=5, sde=True, generator=torch.Generator().manual_seed(42))
    torch.manual_seed(0)
    out = {}
    while pool:
        out.update(pool.step())
    torch.manual_seed(41)
    assert torch.equal(out[h0], dpm.sample_sde(x, steps=5))
    assert torch.equal(out[h1], dpm.sample_sde(x, steps=5, generator=torch.Generator().manual_seed(42)))
    assert not torch.equal(out[h0], out[h1])


# ---- refusals, in order, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if
# any device work preceded them
def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    dpm = _plain()
    with pytest.raises(ValueError, match="sde=True belongs to a slab pool"):
        dpm.request_pool(sde=True)
    with pytest.raises(TypeError):
        SlabPool(dpm)
    pool = dpm.request_pool(slots=8, sde=True)
    # seed rules: RequestPool.submit's
    with pytest.raises(ValueError, match="belong to an SDE request"):
        pool.submit(x, steps=6, seed=1)
    with pytest.raises(ValueError, match="belong to an SDE request"):
        pool.submit(x, steps=6, generator=torch.Generator())
    with pytest.raises(ValueError, match="either `seed` or `generator`"):
        pool.submit(x, steps=6, sde=True, seed=1, generator=torch.Generator())
    for bad in (-1, 1 << 64, 1.5, True):
        with pytest.raises(ValueError, match="`seed` must be"):
            pool.submit(x, steps=6, sde=True, seed=bad)
    # sample_sde's checks of solver and order, then of the state
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, sde=True, seed=1, method="singlestep")
    with pytest.raises(ValueError, match="sample_sde: 'order' must be 1 or 2"):
        pool.submit(x, steps=6, order=3, sde=True, seed=1)
    with pytest.raises(NotImplementedError, match="sample_sde: algorithm_type='dpmsolver'"):
        ns = D.NoiseScheduleVP("linear")
        D.DPM_Solver(D.model_wrapper(_net, ns), ns, algorithm_type="dpmsolver").request_pool(slots=8, sde=True).submit(
            x, steps=6, sde=True, seed=1)
    with pytest.raises(NotImplementedError, match="sample_sde: double-precision states"):
        pool.submit(x.double(), steps=6, sde=True, seed=1)
    with pytest.raises(NotImplementedError, match="slab pool: double-precision states"):
        pool.submit(x.double(), steps=6)
    # a pool without sde=True refuses SDE requests with the text it always had
    with pytest.raises(NotImplementedError, match="sde=True -- SDE stages have no table kernel"):
        dpm.request_pool(slots=8).submit(x, steps=6, sde=True, seed=1)
    # an SDE pool's rows are whole 8-element groups: refused at the first submit, whatever the request's kind
    for kw in (dict(sde=True, seed=1), {}):
        with pytest.raises(NotImplementedError, match="a sample of 12 elements"):
            dpm.request_pool(slots=8, sde=True).submit(torch.randn(2, 3, 2, 2), steps=6, **kw)
    # ... which a well-formed request on the host then meets
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
        pool.submit(x, steps=6, sde=True, seed=1)
    assert not pool and pool.step() == {} and not pool._ropts
