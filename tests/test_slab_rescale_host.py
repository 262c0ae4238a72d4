"""A guidance-rescale slab pool (DPM_Solver.request_pool(slots=S, rescale=True)) and per-request guidance in any classifier-free
slab pool, without a GPU: the host code on the numpy doubles of tests/table_rescale_double.py -- DPM_TABLE_FILL |
DPM_TABLE_RESCALE by the real library, the per-row doubles at LAUNCH (rescale_double.stage for a flagged row, its inputs checked
decidable there: assert_inputs_decidable).  The staggered pool of tests/test_slab_thresh_host.py: requests of 1 and 3 samples,
rows that free up so that a later request lands in non-adjacent rows, every request with a guidance scale and a phi of its own;
every result must be the bits of sample() on the request alone, on a solver whose wrapper has that scale and that phi."""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_rescale_double as TRD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pool_host import NET_CALLS, _net
from test_slab_thresh_host import REQS

FILL_R, LAUNCH_R = L.TABLE_FILL | L.TABLE_RESCALE, L.TABLE_LAUNCH | L.TABLE_RESCALE
SCALES, PHIS = (1.5, 3.0, 7.5), (0.0, 0.7, 1.0)


@pytest.fixture
def doubles(monkeypatch):
    TRD.install_table_rescale_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _solver(dtype, scale=3.0, phi=0.0, cond=None, uncond=None, cfg=True):
    ns = make_schedule("sd")
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if not cfg:
        return D.DPM_Solver(D.model_wrapper(_net, ns), ns, algorithm_type="dpmsolver++", **kw)
    fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=scale,
                         condition=torch.ones(1, 1) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    return D.DPM_Solver(D.cfg_rescale(fn, phi), ns, algorithm_type="dpmsolver++", **kw)


def _guide(j):
    """request j's own (guidance scale, phi); every third request leaves one of the two to the wrapper"""
    return SCALES[j % 3], PHIS[(j + j // 3) % 3]


@pytest.mark.parametrize("wrapper_phi", [0.0, 0.5], ids=["wphi0", "wphi0.5"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_rescale_slab_pool_equals_every_request_alone(doubles, dtype, wrapper_phi):
    g = torch.Generator().manual_seed(213)
    xs = [(2.0 * torch.randn(b, 4, 8, 8, generator=g)).to(dtype) for _, _, b in REQS]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b) in enumerate(REQS)]
    dpm = _solver(dtype, 3.0, wrapper_phi)
    pool = dpm.request_pool(slots=10, rescale=True)
    assert isinstance(pool, SlabPool)
    assert {_guide(j)[1] for j in range(len(REQS))} == set(PHIS) and {_guide(j)[0] for j in range(len(REQS))} == set(SCALES)
    handles, got, rows_of, tick, used = {}, {}, {}, 0, {}
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kw, b) in enumerate(REQS):
            if t == tick:
                s, phi = _guide(j)
                gkw = dict(guidance_scale=s, guidance_rescale=phi)
                if j == 2:
                    del gkw["guidance_scale"]                                    # the wrapper's scale, the request's phi
                    s = 3.0
                if j == 4:
                    del gkw["guidance_rescale"]                                  # the request's scale, the wrapper's phi
                    phi = wrapper_phi
                used[j] = (s, phi)
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], **kw, **gkw)] = j
        nets, calls, launches = len(NET_CALLS), len(TRD.CALLS), len(TRD.ROWS)
        done = pool.step()
        for h, (rws, _) in pool._rows.items():
            rows_of.setdefault(handles[h], list(rws))
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [20]                                      # ONE network call per tick, on the whole slab
            R = TRD.CALLS[calls][0]
            assert TRD.CALLS[calls:] == [(R, FILL_R), (R, LAUNCH_R)]             # exactly two multi-request calls, flagged
            assert len(TRD.ROWS) == launches + 1
        else:
            assert TRD.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(REQS)))
    assert rows_of[5] == [0, 4, 9], rows_of                                     # one request, three non-adjacent rows
    # the rows of the table carried every request's own scale and phi: flagged rows phi in cg_scale, phi 0 rows no flag
    seen = {(np.float32(cs), np.float32(cg)) for _, rows, _ in TRD.ROWS for _, fl, cs, cg in rows if fl & L.F_CFG_RESCALE}
    assert seen == {(np.float32(s), np.float32(phi)) for s, phi in used.values() if phi}
    assert all(fl & L.F_CFG_RESCALE for _, rows, _ in TRD.ROWS for _, fl, _, _ in rows)       # (ten plain rows never fill a run)
    plain = {np.float32(cs) for _, _, reqs in TRD.ROWS for fl, cs, _ in reqs if not fl & L.F_CFG_RESCALE}
    assert plain == {np.float32(s) for s, phi in used.values() if not phi}
    NET_CALLS.clear()
    for j, (_, kw, b) in enumerate(REQS):
        s, phi = used[j]
        alone = _solver(dtype, s, phi, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, s, phi)
    # (the rescale and the scale are there: the same request under the wrapper's own guidance ends elsewhere)
    j = next(j for j in used if used[j][1] == 1.0)
    base = _solver(dtype, used[j][0], 0.0, *[c.expand(REQS[j][2], -1) for c in conds[j]])
    assert not torch.equal(got[j], base.sample(xs[j], **REQS[j][1]))


def test_steady_tick_of_rescale_rows_is_one_run_and_one_copy(doubles):
    dpm = _solver(torch.float32, 7.5, 0.7)
    g = torch.Generator().manual_seed(1)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 8, 8, generator=g) for j in range(10)]
    pool = dpm.request_pool(slots=40, rescale=True)
    hs = [pool.submit(x, steps=8, order=2) for x in xs]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        done.update(pool.step())
    assert pool.copies == 6 and TRD.CALLS[-2:] == [(20, FILL_R), (20, LAUNCH_R)]
    runs, rows, _ = TRD.ROWS[-1]
    assert runs == 1 and len({r[0] for r in rows}) == 20 and all(r[1] & L.F_CFG_RESCALE for r in rows)      # ONE run: one launch
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 40 * L.TABLE_ROW_BYTES + 15) // 16 * 16                     # no further section
    while pool:
        done.update(pool.step())
    for h, x in zip(hs, xs):
        assert torch.equal(done[h], dpm.sample(x, steps=8, order=2))


@pytest.mark.parametrize("kind", ["plain", "unipc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_guidance_scale_per_request_in_a_pool_without_rescale(doubles, dtype, kind):
    g = torch.Generator().manual_seed(7)
    dpm = _solver(dtype, 3.0, 0.0)
    pool = dpm.request_pool(slots=24)
    reqs = [(1 + 2 * (j % 2), SCALES[j % 3] if j % 4 else None, dict(steps=4 + j % 3, order=1 + j % 3 if kind == "plain" else 2))
            for j in range(9)]
    xs = [torch.randn(b, 4, 8, 8, generator=g).to(dtype) for b, _, _ in reqs]
    hs = []
    for x, (b, s, kw) in zip(xs, reqs):
        gkw = {} if s is None else dict(guidance_scale=s)
        hs.append((pool.submit if kind == "plain" else pool.submit_unipc)(x, **kw, **gkw))
    got = {}
    while pool:
        got.update(pool.step())
    assert all(mode & L.TABLE_RESCALE == 0 for _, mode in TRD.CALLS)
    for h, x, (b, s, kw) in zip(hs, xs, reqs):
        alone = _solver(dtype, 3.0 if s is None else s, 0.0)
        want = (alone.sample if kind == "plain" else alone.sample_unipc)(x, **kw)
        assert torch.equal(got[h], want), (b, s, kw)
    assert reqs[2][1] == 7.5                                                      # (the scale is there: the wrapper's ends elsewhere)
    assert not torch.equal(got[hs[2]], (dpm.sample if kind == "plain" else dpm.sample_unipc)(xs[2], **reqs[2][2]))


def test_the_shared_conversion_is_what_planner_and_binder_write():
    """_cfg_fields on a record = the record sample() builds for a wrapper of that scale and phi"""
    from dpm_solver_amd import _device as DV
    x = torch.randn(1, 4, 8, 8)
    for s, phi in ((1.5, 0.0), (7.5, 0.7), (2.25, 1.0)):
        ref = _solver(torch.float32, s, phi)
        base = _solver(torch.float32, 3.0, 0.5)
        a = ref._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, False, "dpmsolver")
        b = base._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, False, "dpmsolver")
        for sa, sb in zip(a.stages, b.stages):
            sa, sb = ref._prep_stage(sa.copy()), base._prep_stage(sb.copy())
            cs, cg, fl = DV._cfg_fields(s, phi, sb.sigma_e, sb.flags)
            assert (np.float32(sa.cfg_scale), np.float32(sa.cg_scale), sa.flags) == (cs, cg, int(fl))


# ---- refusals, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if any device
# work preceded them
def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    dpm, plain, uncond = _solver(torch.float32, 3.0, 0.7), _solver(torch.float32, 3.0, 0.0), _solver(torch.float32, cfg=False)
    with pytest.raises(ValueError, match="rescale=True belongs to a slab pool"):
        dpm.request_pool(rescale=True)
    for kw, text in ((dict(sde=True), "sde=True.*SDE stage kernels have no rescale"),
                     (dict(thresholding=True), "thresholding=True.*thresholding kernels have no rescale"),
                     (dict(inpaint=True), "inpaint=True.*no mask-blend epilogue")):
        with pytest.raises(NotImplementedError, match="rescale=True with " + text):
            dpm.request_pool(slots=8, rescale=True, **kw)
    with pytest.raises(ValueError, match="rescale=True needs a classifier-free wrapper"):
        uncond.request_pool(slots=8, rescale=True)
    with pytest.raises(ValueError, match="rescale=True needs a classifier-free wrapper"):
        _solver(torch.float32, 1.0, 0.7).request_pool(slots=8, rescale=True)          # scale 1: no blend, nothing to rescale
    # without the flag: the refusal a slab pool always gave
    with pytest.raises(NotImplementedError, match="guidance rescale.*slab pool"):
        dpm.request_pool(slots=8)
    pool = dpm.request_pool(slots=8, rescale=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, method="singlestep")
    with pytest.raises(NotImplementedError, match="guidance rescale.*sample_unipc"):      # the wrapper carries phi: as today
        pool.submit_unipc(x, steps=6)
    with pytest.raises(TypeError):
        pool.submit_unipc(x, steps=6, guidance_rescale=0.5)
    # the arguments' own checks
    for bad in ("3", None.__class__, True, float("nan"), 1j):
        with pytest.raises(ValueError, match="guidance_scale must be a real number"):
            pool.submit(x, steps=6, guidance_scale=bad)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"guidance_rescale must be in \[0, 1\]"):
            pool.submit(x, steps=6, guidance_rescale=bad)
    with pytest.raises(ValueError, match="guidance_rescale must be a real number"):
        pool.submit(x, steps=6, guidance_rescale="0.5")
    with pytest.raises(NotImplementedError, match="guidance_scale=1.0.*conditional branch alone"):
        pool.submit(x, steps=6, guidance_scale=1.0)
    with pytest.raises(NotImplementedError, match="guidance_scale=1.0"):
        plain.request_pool(slots=8).submit_unipc(x, steps=6, guidance_scale=1)
    for kw in (dict(guidance_scale=2.0), dict(guidance_rescale=0.5)):
        with pytest.raises(ValueError, match="belong to a classifier-free wrapper"):
            uncond.request_pool(slots=8).submit(x, steps=6, **kw)
    with pytest.raises(ValueError, match="belong to a classifier-free wrapper"):
        uncond.request_pool(slots=8).submit_unipc(x, steps=6, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="guidance_rescale=.*rescale=True"):
        plain.request_pool(slots=8).submit(x, steps=6, guidance_rescale=0.5)
    # the sample has to be a row of the table rescale kernel: refused at the first submit
    for shape, text in (((2, 1, 2, 2), "a sample of 4 elements"), ((2, 3, 2, 2), "a sample of 12 elements"),
                        ((1, 3, 5, 7), "a sample of 105 elements")):
        with pytest.raises(NotImplementedError, match="rescale=True with " + text) as e:
            dpm.request_pool(slots=8, rescale=True).submit(torch.randn(*shape), steps=6)
        assert "request_pool() without slots" in str(e.value)
    # ... which a well-formed request on the host then meets
    for kw in ({}, dict(guidance_scale=7.5, guidance_rescale=0.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
            dpm.request_pool(slots=8, rescale=True).submit(x, steps=6, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
        plain.request_pool(slots=8).submit(x, steps=6, guidance_scale=7.5)
    assert not pool and pool.step() == {}
