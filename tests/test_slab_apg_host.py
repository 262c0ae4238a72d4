"""An adaptive-projected-guidance slab pool (DPM_Solver.request_pool(slots=S, apg=True)) without a GPU: the host code on the
numpy doubles of tests/table_apg_double.py -- DPM_TABLE_FILL | DPM_TABLE_APG by the real library, every APG record checked word
for word at LAUNCH, the per-row doubles (apg_double.stage for a flagged row, its inputs checked decidable there:
assert_inputs_decidable) on the average the row's thr_hint names.  The staggered pool of tests/test_slab_thresh_host.py:
requests of 1 and 3 samples, ten slots for 16 rows' worth of requests, so that requests wait and rows are reused, every
request with a guidance scale and (eta, norm threshold, momentum) of its own; every result must be the bits of sample() on the
request alone, on a solver whose wrapper has that scale and cfg_apg(fn, *its parameters)."""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_apg_double as TAD
from dpm_solver_amd import _device as DV
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pool_host import NET_CALLS, _net
from test_slab_thresh_host import REQS

FILL_A, LAUNCH_A = L.TABLE_FILL | L.TABLE_APG, L.TABLE_LAUNCH | L.TABLE_APG
SCALES = (1.5, 3.0, 7.5)
PARAMS = ((0.0, 15.0, -0.5), (1.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.25, 2.5, 0.25))
PLAIN = (1.0, 0.0, 0.0)


@pytest.fixture
def doubles(monkeypatch):
    TAD.install_table_apg_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _solver(dtype, scale=3.0, apg=None, cond=None, uncond=None, cfg=True, algorithm="dpmsolver++", **skw):
    ns = make_schedule("sd")
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    kw.update(skw)
    if not cfg:
        return D.DPM_Solver(D.model_wrapper(_net, ns), ns, algorithm_type=algorithm, **kw)
    fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=scale,
                         condition=torch.ones(1, 1) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    return D.DPM_Solver(fn if apg is None else D.cfg_apg(fn, *apg), ns, algorithm_type=algorithm, **kw)


def _own(j):
    """request j's own (guidance scale, parameters)"""
    return SCALES[j % 3], PARAMS[(j + 3 * (j // 4)) % 4]


@pytest.mark.parametrize("wrapper_apg", [None, (0.5, 10.0, -0.25)], ids=["wplain", "wapg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_apg_slab_pool_equals_every_request_alone(doubles, dtype, wrapper_apg):
    g = torch.Generator().manual_seed(215)
    xs = [(2.0 * torch.randn(b, 4, 8, 8, generator=g)).to(dtype) for _, _, b in REQS]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b) in enumerate(REQS)]
    dpm = _solver(dtype, 3.0, wrapper_apg)
    pool = dpm.request_pool(slots=10, apg=True)
    assert isinstance(pool, SlabPool)
    assert {_own(j)[1] for j in range(len(REQS))} == set(PARAMS) and {_own(j)[0] for j in range(len(REQS))} == set(SCALES)
    assert any(kw.get("denoise_to_zero") and _own(j)[1][2] != 0 for j, (_, kw, _) in enumerate(REQS))   # DENOISE with a momentum
    handles, got, rows_of, tick, used, admitted_at = {}, {}, {}, 0, {}, {}
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kw, b) in enumerate(REQS):
            if t == tick:
                s, par = _own(j)
                okw = dict(guidance_scale=s, apg=par)
                if j == 2:
                    del okw["guidance_scale"]                                    # the wrapper's scale, the request's parameters
                    s = 3.0
                if j == 6:
                    del okw["apg"]                                               # the request's scale, the wrapper's parameters
                    par = wrapper_apg or PLAIN
                if j == 7:
                    okw = {}                                                     # both the wrapper's
                    s, par = 3.0, wrapper_apg or PLAIN
                used[j] = (s, par)
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], **kw, **okw)] = j
        nets, calls, launches = len(NET_CALLS), len(TAD.CALLS), len(TAD.ROWS)
        done = pool.step()
        for h, (rws, _) in pool._rows.items():
            if handles[h] not in rows_of:
                rows_of[handles[h]], admitted_at[handles[h]] = list(rws), tick
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [20]                                      # ONE network call per tick, on the whole slab
            R = TAD.CALLS[calls][0]
            assert TAD.CALLS[calls:] == [(R, FILL_A), (R, LAUNCH_A)]             # exactly two multi-request calls, flagged
            assert len(TAD.ROWS) == launches + 1
        else:
            assert TAD.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(REQS)))
    # rows were reused, and requests waited for them
    assert any(admitted_at[j] > REQS[j][0] for j in admitted_at), admitted_at
    first = {}
    reused = [j for j in sorted(rows_of, key=lambda j: admitted_at[j]) for r in rows_of[j] if first.setdefault(r, j) != j]
    assert reused, rows_of
    # the table carried every request's own parameters: flagged rows with their record, (1, 0, 0) rows without the flag
    seen = {par for _, rows, _ in TAD.ROWS for _, fl, _, par in rows if fl & L.F_CFG_APG}
    assert seen == {tuple(float(np.float32(v)) for v in par) for _, par in used.values() if par != PLAIN}
    assert all(fl & L.F_CFG_APG for _, rows, _ in TAD.ROWS for _, fl, _, _ in rows)            # (ten plain rows never fill a run)
    plain = {np.float32(cs) for _, _, reqs in TAD.ROWS for fl, cs, *_ in reqs if not fl & L.F_CFG_APG}
    assert plain == {np.float32(s) for s, par in used.values() if par == PLAIN}
    # thr_hint: the row's slice of the pool's average slab where the record has a momentum, null elsewhere
    base, step = pool._avg.data_ptr(), 4 * 8 * 8 * 4
    for _, rows, reqs in TAD.ROWS:
        for fl, _, _, _, beta, hint in reqs:
            mom = bool(fl & L.F_CFG_APG) and beta != 0
            assert (hint != 0) == mom and (not mom or ((hint - base) % step == 0 and 0 <= (hint - base) // step < 10))
        assert all((avg != 0) == (par[2] != 0) for _, fl, avg, par in rows if fl & L.F_CFG_APG)
    NET_CALLS.clear()
    for j, (_, kw, b) in enumerate(REQS):
        s, par = used[j]
        alone = _solver(dtype, s, par, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, s, par)
    # (the projection and the scale are there: the same request under plain guidance of its scale ends elsewhere)
    j = next(j for j in used if used[j][1] == PARAMS[0])
    base_solver = _solver(dtype, used[j][0], None, *[c.expand(REQS[j][2], -1) for c in conds[j]])
    assert not torch.equal(got[j], base_solver.sample(xs[j], **REQS[j][1]))


@pytest.mark.parametrize("b", [1, 2])
def test_a_reused_row_starts_from_a_zero_average(doubles, b):
    """two slots, two momentum requests of the same rows one after the other: the second must not see the first's average"""
    g = torch.Generator().manual_seed(3)
    par = (0.0, 15.0, -0.5)
    dpm = _solver(torch.float32, 7.5, par)
    xa, xb = 2.0 * torch.randn(2, 4, 8, 8, generator=g), 2.0 * torch.randn(b, 4, 8, 8, generator=g)
    pool = dpm.request_pool(slots=2, apg=True)
    ha, hb = pool.submit(xa, steps=4, order=2), pool.submit(xb, steps=5, order=2, apg=(0.5, 0.0, -0.75))
    got, left = {}, None
    while pool:
        if hb not in pool._rows and ha not in pool._rows and ha in got and left is None:
            left = pool._avg.clone()                                              # what request A left in the rows B will take
        got.update(pool.step())
        assert ha in got or hb not in pool._rows                                  # B waited for A's rows
    assert left is not None and bool((left[:b] != 0).any()), "the first request left no average: the test shows nothing"
    assert torch.equal(got[ha], dpm.sample(xa, steps=4, order=2))
    alone = _solver(torch.float32, 7.5, (0.5, 0.0, -0.75))
    assert torch.equal(got[hb], alone.sample(xb, steps=5, order=2))


def test_steady_tick_of_apg_rows_is_one_run_and_one_copy(doubles):
    dpm = _solver(torch.float32, 7.5, (0.0, 15.0, -0.5))
    g = torch.Generator().manual_seed(1)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 8, 8, generator=g) for j in range(10)]
    pool = dpm.request_pool(slots=40, apg=True)
    hs = [pool.submit(x, steps=8, order=2, **(dict(apg=(0.5, 0.0, 0.0)) if j % 3 == 0 else {})) for j, x in enumerate(xs)]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        nets = len(NET_CALLS)
        done.update(pool.step())
        assert len(NET_CALLS) == nets + 1
    assert pool.copies == 6 and TAD.CALLS[-2:] == [(20, FILL_A), (20, LAUNCH_A)]
    runs, rows, _ = TAD.ROWS[-1]
    # ONE run, one launch: rows with and without a momentum share it
    assert runs == 1 and len({r[0] for r in rows}) == 20 and all(r[1] & L.F_CFG_APG for r in rows)
    assert {r[3][2] != 0 for r in rows} == {True, False}
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 40 * (L.TABLE_ROW_BYTES + L.TABLE_APG_BYTES) + 15) // 16 * 16
    assert pool._tabb == (L.table_bytes(40, L.TABLE_APG) + 15) // 16 * 16
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        alone = _solver(torch.float32, 7.5, (0.5, 0.0, 0.0)) if j % 3 == 0 else dpm
        assert torch.equal(done[h], alone.sample(x, steps=8, order=2))


def test_the_shared_conversion_is_what_the_binder_writes():
    """_apg_fields over the plain record = the record sample() builds for a wrapper of those parameters"""
    x = torch.randn(1, 4, 8, 8)
    for par in ((0.0, 15.0, -0.5), (0.5, 0.0, 0.0), PLAIN, (1.0, 0.0, 0.3)):
        ref, base = _solver(torch.float32, 3.0, par), _solver(torch.float32, 3.0, None)
        a = ref._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
        b = base._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
        for sa, sb in zip(a.stages, b.stages):
            sa, sb = ref._prep_stage(sa.copy()), base._prep_stage(sb.copy())
            cg, ratio, mx, fl = DV._apg_fields(*par, (sb.cg_scale, sb.thr_ratio, sb.thr_max), sb.flags)
            assert (np.float32(sa.cg_scale), np.float32(sa.thr_ratio), np.float32(sa.thr_max), sa.flags) == (cg, ratio, mx, int(fl))
            assert bool(sa.flags & L.F_CFG_APG) == (par != PLAIN)


# ---- refusals, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if any device
# work preceded them
def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    par = (0.0, 15.0, -0.5)
    dpm, plain, uncond = _solver(torch.float32, 3.0, par), _solver(torch.float32, 3.0, None), _solver(torch.float32, cfg=False)
    with pytest.raises(ValueError, match="apg=True belongs to a slab pool"):
        dpm.request_pool(apg=True)
    for kw, text in ((dict(rescale=True), "rescale=True.*APG kernel has no guidance rescale"),
                     (dict(sde=True), "sde=True.*APG kernel has no noise epilogue"),
                     (dict(thresholding=True), "thresholding=True.*APG kernel has no thresholding"),
                     (dict(inpaint=True), "inpaint=True.*APG kernel has no mask-blend epilogue")):
        with pytest.raises(NotImplementedError, match="apg=True with " + text):
            plain.request_pool(slots=8, apg=True, **kw)
    with pytest.raises(ValueError, match="apg=True needs a classifier-free wrapper"):
        uncond.request_pool(slots=8, apg=True)
    with pytest.raises(ValueError, match="apg=True needs a classifier-free wrapper"):
        _solver(torch.float32, 1.0, None).request_pool(slots=8, apg=True)             # scale 1: no direction to project
    with pytest.raises(NotImplementedError, match="apg=True with algorithm_type='dpmsolver'.*data prediction"):
        _solver(torch.float32, 3.0, None, algorithm="dpmsolver").request_pool(slots=8, apg=True)
    with pytest.raises(NotImplementedError, match="apg=True on a solver with correcting_x0_fn='dynamic_thresholding'"):
        _solver(torch.float32, 3.0, None, correcting_x0_fn="dynamic_thresholding").request_pool(slots=8, apg=True)
    # without the flag: the refusal a slab pool always gave
    with pytest.raises(NotImplementedError, match="adaptive projected guidance.*slab pool"):
        dpm.request_pool(slots=8)
    pool = dpm.request_pool(slots=8, apg=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, method="singlestep")
    with pytest.raises(NotImplementedError, match="adaptive projected guidance.*sample_unipc"):     # the wrapper carries APG: as today
        pool.submit_unipc(x, steps=6)
    with pytest.raises(TypeError):
        pool.submit_unipc(x, steps=6, apg=par)
    # the argument's own checks: cfg_apg's ranges and texts
    for bad in ("0.5", None.__class__, True, float("nan"), 1j):
        with pytest.raises(ValueError, match="cfg_apg: eta must be a real number"):
            pool.submit(x, steps=6, apg=(bad, 0.0, 0.0))
    with pytest.raises(ValueError, match="cfg_apg: norm_threshold must be a real number"):
        pool.submit(x, steps=6, apg=(0.5, "1", 0.0))
    with pytest.raises(ValueError, match="cfg_apg: momentum must be a real number"):
        pool.submit(x, steps=6, apg=(0.5, 1.0, None))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"cfg_apg: eta must be in \[0, 1\]"):
            pool.submit(x, steps=6, apg=(bad, 0.0, 0.0))
    for bad in (-1.0, float("inf")):
        with pytest.raises(ValueError, match="cfg_apg: norm_threshold must be a finite number >= 0"):
            pool.submit(x, steps=6, apg=(0.5, bad, 0.0))
    for bad in (-1.0, 1.0, 2.0):
        with pytest.raises(ValueError, match=r"cfg_apg: momentum must be in \(-1, 1\)"):
            pool.submit(x, steps=6, apg=(0.5, 0.0, bad))
    for bad in (0.5, (0.5, 0.0), "abc", (0.5, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match=r"apg= takes \(eta, norm_threshold, momentum\)"):
            pool.submit(x, steps=6, apg=bad)
    with pytest.raises(NotImplementedError, match="guidance_scale=1.0.*conditional branch alone"):
        pool.submit(x, steps=6, guidance_scale=1.0, apg=par)
    with pytest.raises(NotImplementedError, match="guidance_rescale=.*rescale=True"):
        pool.submit(x, steps=6, guidance_rescale=0.5)
    with pytest.raises(ValueError, match="apg= belongs to a classifier-free wrapper"):
        uncond.request_pool(slots=8).submit(x, steps=6, apg=par)
    with pytest.raises(NotImplementedError, match="apg= .*apg=True"):
        plain.request_pool(slots=8).submit(x, steps=6, apg=par)
    # the sample has to be a row of the table APG kernel: refused at the first submit
    for shape, text in (((2, 1, 2, 2), "a sample of 4 elements"), ((2, 3, 2, 2), "a sample of 12 elements"),
                        ((1, 3, 5, 7), "a sample of 105 elements")):
        with pytest.raises(NotImplementedError, match="apg=True with " + text) as e:
            dpm.request_pool(slots=8, apg=True).submit(torch.randn(*shape), steps=6)
        assert "request_pool() without slots" in str(e.value)
    # ... which a well-formed request on the host then meets
    for kw in ({}, dict(guidance_scale=7.5, apg=PLAIN), dict(apg=(0.5, 0.0, 0.25))):
        with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
            dpm.request_pool(slots=8, apg=True).submit(x, steps=6, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
        plain.request_pool(slots=8, apg=True).submit(x, steps=6, apg=par)
    assert not pool and pool.step() == {}
