"""A CFG-Zero* slab pool (DPM_Solver.request_pool(slots=S, zero_star=True)) without a GPU: the host code on the numpy doubles
of tests/table_zstar_double.py -- DPM_TABLE_FILL | DPM_TABLE_ZSTAR by the real library, the per-row doubles at LAUNCH
(zstar_double.stage for a flagged row, its inputs checked decidable there: assert_inputs_decidable).  The staggered pool of
tests/test_slab_thresh_host.py: requests of 1 and 3 samples, ten slots for 16 rows' worth of requests, so that requests wait
and rows are reused, every request with a guidance scale and a choice of its own; every result must be the bits of sample() on
the request alone, on a solver whose wrapper has that scale and cfg_zero_star (or not)."""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_zstar_double as TZD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pool_host import NET_CALLS, _net
from test_slab_thresh_host import REQS

FILL_Z, LAUNCH_Z = L.TABLE_FILL | L.TABLE_ZSTAR, L.TABLE_LAUNCH | L.TABLE_ZSTAR
SCALES = (1.5, 3.0, 7.5)


@pytest.fixture
def doubles(monkeypatch):
    TZD.install_table_zstar_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _solver(dtype, scale=3.0, zstar=False, cond=None, uncond=None, cfg=True, remedy=None, **skw):
    ns = make_schedule("sd")
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    kw.update(skw)
    kw.setdefault("algorithm_type", "dpmsolver++")
    if not cfg:
        return D.DPM_Solver(D.model_wrapper(_net, ns), ns, **kw)
    fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=scale,
                         condition=torch.ones(1, 1) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    if remedy is not None:
        fn = remedy(fn)
    return D.DPM_Solver(D.cfg_zero_star(fn) if zstar else fn, ns, **kw)


def _own(j):
    """request j's own (guidance scale, choice)"""
    return SCALES[j % 3], (True, False, True, True)[(j + j // 4 + 1) % 4]


@pytest.mark.parametrize("wrapper_zstar", [False, True], ids=["wplain", "wzstar"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_zstar_slab_pool_equals_every_request_alone(doubles, dtype, wrapper_zstar):
    g = torch.Generator().manual_seed(217)
    xs = [(2.0 * torch.randn(b, 4, 8, 8, generator=g)).to(dtype) for _, _, b in REQS]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b) in enumerate(REQS)]
    dpm = _solver(dtype, 3.0, wrapper_zstar)
    pool = dpm.request_pool(slots=10, zero_star=True)
    assert isinstance(pool, SlabPool)
    assert {_own(j)[1] for j in range(len(REQS))} == {True, False} and {_own(j)[0] for j in range(len(REQS))} == set(SCALES)
    assert any(kw.get("denoise_to_zero") and _own(j)[1] for j, (_, kw, _) in enumerate(REQS))       # DENOISE under the flag
    handles, got, rows_of, tick, used, admitted_at = {}, {}, {}, 0, {}, {}
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kw, b) in enumerate(REQS):
            if t == tick:
                s, on = _own(j)
                okw = dict(guidance_scale=s, zero_star=on)
                if j == 2:
                    del okw["guidance_scale"]                                    # the wrapper's scale, the request's choice
                    s = 3.0
                if j == 6:
                    del okw["zero_star"]                                         # the request's scale, the wrapper's choice
                    on = wrapper_zstar
                if j == 7:
                    okw = {}                                                     # both the wrapper's
                    s, on = 3.0, wrapper_zstar
                used[j] = (s, on)
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], **kw, **okw)] = j
        nets, calls, launches = len(NET_CALLS), len(TZD.CALLS), len(TZD.ROWS)
        done = pool.step()
        for h, (rws, _) in pool._rows.items():
            if handles[h] not in rows_of:
                rows_of[handles[h]], admitted_at[handles[h]] = list(rws), tick
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [20]                                      # ONE network call per tick, on the whole slab
            R = TZD.CALLS[calls][0]
            assert TZD.CALLS[calls:] == [(R, FILL_Z), (R, LAUNCH_Z)]             # exactly two multi-request calls, flagged
            assert len(TZD.ROWS) == launches + 1
        else:
            assert TZD.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(REQS)))
    # rows were reused, and requests waited for them
    assert any(admitted_at[j] > REQS[j][0] for j in admitted_at), admitted_at
    first = {}
    reused = [j for j in sorted(rows_of, key=lambda j: admitted_at[j]) for r in rows_of[j] if first.setdefault(r, j) != j]
    assert reused, rows_of
    # the table carried every request's own scale: flagged requests own rows, the others carry no flag and (ten plain rows never
    # fill a run) own none
    seen = {np.float32(cs) for _, rows, _ in TZD.ROWS for _, fl, cs in rows}
    assert seen == {np.float32(s) for s, on in used.values() if on}
    assert all(fl & L.F_CFG_ZSTAR for _, rows, _ in TZD.ROWS for _, fl, _ in rows)
    for runs, rows, reqs in TZD.ROWS:
        assert len(rows) == sum(1 for fl, _ in reqs if fl & L.F_CFG_ZSTAR) and runs == (1 if rows else 0)
    plain = {np.float32(cs) for _, _, reqs in TZD.ROWS for fl, cs in reqs if not fl & L.F_CFG_ZSTAR}
    assert plain == {np.float32(s) for s, on in used.values() if not on}
    NET_CALLS.clear()
    for j, (_, kw, b) in enumerate(REQS):
        s, on = used[j]
        alone = _solver(dtype, s, on, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, s, on)
    # (the projection is there: the same request under plain guidance of its scale ends elsewhere)
    j = next(j for j in used if used[j][1])
    base = _solver(dtype, used[j][0], False, *[c.expand(REQS[j][2], -1) for c in conds[j]])
    assert not torch.equal(got[j], base.sample(xs[j], **REQS[j][1]))


def test_a_request_without_the_projection_is_the_plain_solvers(doubles):
    """zero_star=False in a pool whose wrapper has the setting: the plain solver's result, and no flagged record for it"""
    g = torch.Generator().manual_seed(5)
    dpm, plain = _solver(torch.float32, 7.5, True), _solver(torch.float32, 7.5, False)
    xa, xb = 2.0 * torch.randn(2, 4, 8, 8, generator=g), 2.0 * torch.randn(1, 4, 8, 8, generator=g)
    pool = dpm.request_pool(slots=4, zero_star=True)
    ha = pool.submit(xa, steps=5, order=2, zero_star=False)
    got = {}
    for _ in range(2):
        got.update(pool.step())
    assert all(not fl & L.F_CFG_ZSTAR for _, _, reqs in TZD.ROWS for fl, _ in reqs) and all(not rows for _, rows, _ in TZD.ROWS)
    hb = pool.submit(xb, steps=4, order=2, denoise_to_zero=True)                 # the wrapper's: flagged
    x_a = {int(pool._x[k].data_ptr()) + r * pool._rowb for k in (0, 1) for r in pool._rows[ha][0]}
    n0 = len(TZD.ROWS)
    while pool:
        got.update(pool.step())
    for _, rows, reqs in TZD.ROWS[n0:]:
        assert all(x not in x_a for x, _, _ in rows)                             # request A never owns a CFG-Zero* row
        assert all(fl & L.F_CFG_ZSTAR for _, fl, _ in rows)
    assert any(rows for _, rows, _ in TZD.ROWS[n0:])
    assert torch.equal(got[ha], plain.sample(xa, steps=5, order=2))
    assert torch.equal(got[hb], dpm.sample(xb, steps=4, order=2, denoise_to_zero=True))
    assert not torch.equal(got[ha], dpm.sample(xa, steps=5, order=2))


def test_a_pool_without_the_switch_never_sends_the_flag(doubles):
    dpm = _solver(torch.float32, 3.0, False)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(1 + j % 2, 4, 8, 8, generator=g) for j in range(4)]
    pool = dpm.request_pool(slots=8)
    hs = [pool.submit(x, steps=4, order=2, **(dict(zero_star=False) if j % 2 else {})) for j, x in enumerate(xs)]
    got = {}
    while pool:
        got.update(pool.step())
    assert TZD.CALLS and all(mode & L.TABLE_ZSTAR == 0 for _, mode in TZD.CALLS)
    assert all(not fl & L.F_CFG_ZSTAR for _, _, reqs in TZD.ROWS for fl, _ in reqs)
    for h, x in zip(hs, xs):
        assert torch.equal(got[h], dpm.sample(x, steps=4, order=2))


def test_steady_tick_of_zstar_rows_is_one_run_and_one_copy(doubles):
    dpm = _solver(torch.float32, 7.5, True)
    g = torch.Generator().manual_seed(1)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 8, 8, generator=g) for j in range(10)]
    pool = dpm.request_pool(slots=40, zero_star=True)
    hs = [pool.submit(x, steps=8, order=2) for x in xs]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        nets = len(NET_CALLS)
        done.update(pool.step())
        assert len(NET_CALLS) == nets + 1
    assert pool.copies == 6 and TZD.CALLS[-2:] == [(20, FILL_Z), (20, LAUNCH_Z)]
    runs, rows, _ = TZD.ROWS[-1]
    assert runs == 1 and len({r[0] for r in rows}) == 20 and all(r[1] & L.F_CFG_ZSTAR for r in rows)        # ONE run: one launch
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 40 * L.TABLE_ROW_BYTES + 15) // 16 * 16                     # no further section
    assert pool._tabb == (L.table_bytes(40, L.TABLE_ZSTAR) + 15) // 16 * 16
    while pool:
        done.update(pool.step())
    for h, x in zip(hs, xs):
        assert torch.equal(done[h], dpm.sample(x, steps=8, order=2))


def test_the_tick_writes_what_the_binder_writes():
    """the flag over the plain record = the record sample() builds for a wrapper with the setting"""
    x = torch.randn(1, 4, 8, 8)
    ref, base = _solver(torch.float32, 3.0, True), _solver(torch.float32, 3.0, False)
    a = ref._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
    b = base._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
    for sa, sb in zip(a.stages, b.stages):
        sa, sb = ref._prep_stage(sa.copy()), base._prep_stage(sb.copy())
        assert sa.flags == sb.flags | L.F_CFG_ZSTAR and sb.flags & L.F_CFG_ZSTAR == 0
        sb.flags |= L.F_CFG_ZSTAR
        assert bytes(sa) == bytes(sb)                                             # the flag and nothing else


# ---- refusals, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if any device
# work preceded them
def _raises(exc, text):
    """the FULL message"""
    import re
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    dpm, plain, uncond = _solver(torch.float32, 3.0, True), _solver(torch.float32, 3.0, False), _solver(torch.float32, cfg=False)
    with _raises(ValueError, "request_pool: zero_star=True belongs to a slab pool (slots=...); a RequestPool takes a cfg_zero_star "
                             "solver as it is"):
        dpm.request_pool(zero_star=True)
    for other, why in (("rescale", "the CFG-Zero* kernel has no guidance rescale"),
                       ("apg", "the CFG-Zero* kernel has no projected guidance"),
                       ("sde", "the CFG-Zero* kernel has no noise epilogue"),
                       ("thresholding", "the CFG-Zero* kernel has no thresholding"),
                       ("inpaint", "the CFG-Zero* kernel has no mask-blend epilogue")):
        with _raises(NotImplementedError, "request_pool: zero_star=True with %s=True -- %s (a follow-up)" % (other, why)):
            plain.request_pool(slots=8, zero_star=True, **{other: True})
    needs = ("request_pool: zero_star=True needs a classifier-free wrapper (an unconditional condition and a guidance scale "
             "other than 1): CFG-Zero* projects the unconditional output onto the conditional one")
    with _raises(ValueError, needs):
        uncond.request_pool(slots=8, zero_star=True)
    with _raises(ValueError, needs):
        _solver(torch.float32, 1.0, False).request_pool(slots=8, zero_star=True)      # scale 1: no blend, nothing to project
    for remedy, name in ((lambda fn: D.cfg_rescale(fn, 0.7), "cfg_rescale"), (lambda fn: D.cfg_apg(fn, 0.0, 15.0, -0.5), "cfg_apg")):
        with _raises(NotImplementedError, "request_pool: zero_star=True on a solver with %s -- the CFG-Zero* kernel has none of "
                                          "those epilogues (a follow-up)" % name):
            _solver(torch.float32, 3.0, False, remedy=remedy).request_pool(slots=8, zero_star=True)
    # a thresholding solver: the pool's own refusal, at submit, as for every pool built without thresholding=True
    with _raises(NotImplementedError, "slab pool: correcting_x0_fn='dynamic_thresholding' -- thresholded stages have no table "
                                      "kernel; use request_pool() without slots"):
        _solver(torch.float32, 3.0, False, correcting_x0_fn="dynamic_thresholding").request_pool(slots=8, zero_star=True).submit(x, steps=6)
    # without the switch: the refusal a slab pool always gave, whatever other switch is on
    slab = ("CFG-Zero* (cfg_zero_star): the slab pool (request_pool(slots=...)) -- CFG-Zero* stages have no table row kind yet (a "
            "follow-up); a RequestPool (no slots) takes a cfg_zero_star solver as it is")
    for kw in ({}, dict(rescale=True), dict(apg=True)):
        with _raises(NotImplementedError, slab):
            dpm.request_pool(slots=8, **kw)
    pool = dpm.request_pool(slots=8, zero_star=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, method="singlestep")
    with pytest.raises(NotImplementedError, match=r"^CFG-Zero\* \(cfg_zero_star\): sample_unipc"):   # the wrapper carries it: as today
        pool.submit_unipc(x, steps=6)
    with pytest.raises(TypeError):
        pool.submit_unipc(x, steps=6, zero_star=True)
    # the argument's own checks
    for bad in (1, 0, "True", 1.0, (True,)):
        with _raises(ValueError, "slab pool: zero_star= takes True or False, got %r" % (bad,)):
            pool.submit(x, steps=6, zero_star=bad)
    with _raises(ValueError, "slab pool: zero_star= belongs to a classifier-free wrapper (with an unconditional condition and a "
                             "guidance scale other than 1)"):
        uncond.request_pool(slots=8).submit(x, steps=6, zero_star=True)
    with _raises(NotImplementedError, "slab pool: zero_star= -- CFG-Zero* stages take the table in a pool built with "
                                      "request_pool(slots=..., zero_star=True) only"):
        plain.request_pool(slots=8).submit(x, steps=6, zero_star=True)
    with pytest.raises(NotImplementedError, match="guidance_scale=1.0.*conditional branch alone"):
        pool.submit(x, steps=6, guidance_scale=1.0, zero_star=True)
    with pytest.raises(NotImplementedError, match="guidance_rescale=.*rescale=True"):
        pool.submit(x, steps=6, guidance_rescale=0.5)
    with pytest.raises(NotImplementedError, match="apg= .*apg=True"):
        pool.submit(x, steps=6, apg=(0.5, 0.0, 0.0))
    # the sample has to be a row of the table CFG-Zero* kernel: refused at the first submit
    for shape, per in (((2, 1, 2, 2), 4), ((2, 3, 2, 2), 12), ((1, 3, 5, 7), 105)):
        with _raises(NotImplementedError, "slab pool: zero_star=True with a sample of %d elements -- a CFG-Zero* row of the table "
                                          "is whole 8-element groups of 16-byte aligned buffers; use request_pool() without "
                                          "slots" % per):
            dpm.request_pool(slots=8, zero_star=True).submit(torch.randn(*shape), steps=6)
    # ... which a well-formed request on the host then meets
    for kw in ({}, dict(guidance_scale=7.5, zero_star=False), dict(zero_star=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
            dpm.request_pool(slots=8, zero_star=True).submit(x, steps=6, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
        plain.request_pool(slots=8, zero_star=True).submit(x, steps=6, zero_star=True)
    assert not pool and pool.step() == {}
