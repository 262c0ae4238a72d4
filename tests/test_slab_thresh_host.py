"""A thresholding slab pool (DPM_Solver.request_pool(slots=S, thresholding=True)) without a GPU: its host code on the numpy
doubles of tests/table_thresh_double.py -- DPM_TABLE_FILL | DPM_TABLE_THRESH by the real library, the per-row doubles at
LAUNCH.  A staggered pool of thresholded requests of 1 and 3 samples; rows free up so that a later request lands in
non-adjacent rows, and every result must still be the bits of sample() on the request alone."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_thresh_double as TTD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pool_host import NET_CALLS, _net

FILL_T, LAUNCH_T = L.TABLE_FILL | L.TABLE_THRESH, L.TABLE_LAUNCH | L.TABLE_THRESH


@pytest.fixture
def doubles(monkeypatch):
    TTD.install_table_thresh_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _solver(cfg, dtype, thresholding=True, cond=None, uncond=None):
    ns = make_schedule("sd")
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_net, ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++",
                        correcting_x0_fn="dynamic_thresholding" if thresholding else None, **kw)


# (tick of submission, kwargs, b).  Tick 0 fills rows 0..8 of 10; the requests of rows 0 and 4 finish after three ticks, so the
# three samples of request 5 land in rows 0, 4 and 9; request 6 finds no free rows and waits.
REQS = [
    (0, dict(steps=3, order=2), 1),
    (0, dict(steps=9, order=2), 3),
    (0, dict(steps=3, order=1), 1),
    (0, dict(steps=8, order=3, skip_type="logSNR"), 3),
    (0, dict(steps=7, order=2, denoise_to_zero=True), 1),
    (3, dict(steps=5, order=3), 3),
    (3, dict(steps=4, order=2, skip_type="time_quadratic"), 3),
    (5, dict(steps=6, order=1), 1),
]


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_thresholding_slab_pool_equals_every_request_alone(doubles, dtype, cfg):
    g = torch.Generator().manual_seed(210)
    xs = [(2.0 * torch.randn(b, 4, 8, 8, generator=g)).to(dtype) for _, _, b in REQS]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b) in enumerate(REQS)]
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=10, thresholding=True)
    assert isinstance(pool, SlabPool)
    handles, got, rows_of, tick = {}, {}, {}, 0
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kw, b) in enumerate(REQS):
            if t == tick:
                ckw = dict(condition=conds[j][0], unconditional_condition=conds[j][1]) if cfg else {}
                handles[pool.submit(xs[j], **kw, **ckw)] = j
        nets, calls, launches = len(NET_CALLS), len(TTD.CALLS), len(TTD.ROWS)
        done = pool.step()
        for h, (rws, _) in pool._rows.items():
            rows_of.setdefault(handles[h], list(rws))
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [20 if cfg else 10]                      # ONE network call per tick, on the whole slab
            R = TTD.CALLS[calls][0]
            assert TTD.CALLS[calls:] == [(R, FILL_T), (R, LAUNCH_T)]            # exactly two multi-request calls, flagged
            runs, xptrs = TTD.ROWS[launches]
            assert len(TTD.ROWS) == launches + 1 and runs == 1                  # every active row in ONE run: one launch
            assert len(set(xptrs)) == R and 0 not in xptrs
        else:
            assert TTD.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(REQS)))
    assert rows_of[5] == [0, 4, 9], rows_of                                     # one request, three non-adjacent rows
    NET_CALLS.clear()
    for j, (_, kw, b) in enumerate(REQS):
        alone = _solver(cfg, dtype, True, *[c.expand(b, -1) for c in conds[j]]) if cfg else dpm
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b)
    # (the thresholding is there: the same request without it ends elsewhere)
    plain = _solver(cfg, dtype, False, *[c.expand(1, -1) for c in conds[0]]) if cfg else _solver(cfg, dtype, False)
    assert not torch.equal(got[0], plain.sample(xs[0], **REQS[0][1]))


def test_steady_state_is_one_copy_per_tick(doubles):
    dpm = _solver(False, torch.float32)
    g = torch.Generator().manual_seed(1)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 8, 8, generator=g) for j in range(10)]
    pool = dpm.request_pool(slots=40, thresholding=True)
    hs = [pool.submit(x, steps=8, order=2) for x in xs]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        done.update(pool.step())
    assert pool.copies == 6 and TTD.CALLS[-2:] == [(20, FILL_T), (20, LAUNCH_T)]
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 40 * L.TABLE_ROW_BYTES + 15) // 16 * 16      # no further section
    while pool:
        done.update(pool.step())
    for h, x in zip(hs, xs):
        assert torch.equal(done[h], dpm.sample(x, steps=8, order=2))


# ---- refusals, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if any device
# work preceded them
def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    dpm = _solver(False, torch.float32)
    with pytest.raises(ValueError, match="thresholding=True on a solver built without"):
        _solver(False, torch.float32, thresholding=False).request_pool(slots=8, thresholding=True)
    with pytest.raises(ValueError, match="thresholding=True belongs to a slab pool"):
        dpm.request_pool(thresholding=True)
    # without the flag: the refusal a slab pool always gave
    with pytest.raises(NotImplementedError, match="thresholded stages have no table kernel"):
        dpm.request_pool(slots=8).submit(x, steps=6)
    pool = dpm.request_pool(slots=8, thresholding=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, method="singlestep")
    # UniPC and SDE: refused by their own checks of a thresholding solver
    with pytest.raises(NotImplementedError):
        pool.submit_unipc(x, steps=6)
    with pytest.raises(NotImplementedError):
        dpm.request_pool(slots=8, sde=True, thresholding=True).submit(x, steps=6, sde=True, seed=1)
    # the sample has to fit a row of the table thresholding kernel: refused at the first submit
    for shape, text in (((1, 3, 64, 65), "a sample of 12480 elements"), ((2, 3, 2, 2), "a sample of 12 elements"),
                        ((1, 12296), "a sample of 12296 elements")):
        with pytest.raises(NotImplementedError, match=text) as e:
            dpm.request_pool(slots=8, thresholding=True).submit(torch.randn(*shape), steps=6)
        assert "request_pool() without slots" in str(e.value)
    # ... which a well-formed request on the host then meets ([3,64,64] is exactly 12288)
    for ok in (x, torch.randn(1, 3, 64, 64)):
        with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
            dpm.request_pool(slots=8, thresholding=True).submit(ok, steps=6)
    assert not pool and pool.step() == {}
