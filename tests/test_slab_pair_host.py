"""A two-condition slab pool (DPM_Solver.request_pool(slots=S, pair=True)) without a GPU: the host code on the numpy doubles of
tests/table_pair_double.py -- DPM_TABLE_FILL | DPM_TABLE_PAIR by the real library, the per-row doubles at LAUNCH
(pair_double.stage, then the two copies).  A staggered pool: 8 rows, 12 requests of 1 and 3 samples, steps 4..9, orders 1..3, so
that requests wait and rows are reused; every request brings its own conditions, second condition, guidance scale and
(scale2, nested); every result must be the bits of sample() on the request alone, on a solver whose wrapper is
cfg_pair(model_wrapper(..., guidance_scale=s, condition=c, unconditional_condition=u), c2, scale2, nested)."""
import re

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_pair_double as TPD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pool_host import NET_CALLS, _net

FILL_P, LAUNCH_P = L.TABLE_FILL | L.TABLE_PAIR, L.TABLE_LAUNCH | L.TABLE_PAIR
SLOTS = 8
# (tick of submission, sample() kwargs, b): steps 4..9, orders 1..3, b in {1, 3}; request 4 ends with the DENOISE stage
REQS = [(j // 3, dict(steps=4 + j % 6, order=1 + j % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 1],
                      denoise_to_zero=(j == 4)), (1, 3)[j % 3 == 2]) for j in range(12)]
# request j's own (s, scale2, nested): guidance scale 1.0 among them (a pair wrapper always evaluates three branches)
OWN = [((1.0, 1.5, 3.0, 7.5)[j % 4], (0.75, 2.5, 1.25)[j % 3], bool(j % 2)) for j in range(12)]


@pytest.fixture
def doubles(monkeypatch):
    TPD.install_table_pair_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _solver(dtype=torch.float32, s=3.0, scale2=1.5, nested=False, cond=None, uncond=None, cond2=None, pair=True, **skw):
    ns = make_schedule("sd")
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    kw.update(skw)
    kw.setdefault("algorithm_type", "dpmsolver++")
    fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=s,
                         condition=torch.ones(1, 1) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    if pair:
        fn = D.cfg_pair(fn, torch.full((1, 1), 0.5) if cond2 is None else cond2, scale2, nested)
    return D.DPM_Solver(fn, ns, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_pair_slab_pool_equals_every_request_alone(doubles, dtype):
    g = torch.Generator().manual_seed(219)
    xs = [(2.0 * torch.randn(b, 4, 8, 8, generator=g)).to(dtype) for _, _, b in REQS]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0,
              torch.rand(b if j % 4 == 2 else 1, 1, generator=g) + 0.5) for j, (_, _, b) in enumerate(REQS)]
    dpm = _solver(dtype)
    pool = dpm.request_pool(slots=SLOTS, pair=True)
    assert isinstance(pool, SlabPool)
    assert {b for _, _, b in REQS} == {1, 3} and {kw["steps"] for _, kw, _ in REQS} == set(range(4, 10))
    assert {kw["order"] for _, kw, _ in REQS} == {1, 2, 3} and sum(kw["denoise_to_zero"] for _, kw, _ in REQS) == 1
    assert {n for _, _, n in OWN} == {True, False} and any(s == 1.0 for s, _, _ in OWN)
    handles, got, rows_of, admitted_at, tick, used = {}, {}, {}, {}, 0, {}
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kw, b) in enumerate(REQS):
            if t == tick:
                s, scale2, nested = OWN[j]
                okw = dict(guidance_scale=s, pair=(scale2, nested))
                if j == 3:
                    del okw["guidance_scale"]                    # the wrapper's scale, the request's second scale
                    s = 3.0
                if j == 7:
                    okw = {}                                     # both the wrapper's
                    s, scale2, nested = 3.0, 1.5, False
                used[j] = (s, scale2, nested)
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], condition2=conds[j][2],
                                    **kw, **okw)] = j
        nets, calls, launches = len(NET_CALLS), len(TPD.CALLS), len(TPD.ROWS)
        done = pool.step()
        for h, (rws, _) in pool._rows.items():
            if handles[h] not in rows_of:
                rows_of[handles[h]], admitted_at[handles[h]] = list(rws), tick
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [3 * SLOTS]               # ONE network call per tick, on the whole [3S] slab
            R = TPD.CALLS[calls][0]
            assert TPD.CALLS[calls:] == [(R, FILL_P), (R, LAUNCH_P)]
            assert len(TPD.ROWS) == launches + 1
            runs, rows = TPD.ROWS[-1]
            assert len(rows) == R and 1 <= runs <= 2             # every active row is a pair row (a last stage under
        else:                                                    # denoise_to_zero differs in DPM_F_TO_X0: a run of its own)
            assert TPD.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(REQS)))
    assert any(admitted_at[j] > REQS[j][0] for j in admitted_at), admitted_at      # requests waited for rows ...
    first = {}
    reused = [j for j in sorted(rows_of, key=lambda j: admitted_at[j]) for r in rows_of[j] if first.setdefault(r, j) != j]
    assert reused, rows_of                                                         # ... and rows were reused
    # the table carried every request's own two scales, formed as cfg_pair and _prep_stage form them
    want = {(float(np.float32(s)), float(np.float32(sc2 - s if nested else sc2))) for s, sc2, nested in used.values()}
    assert {(s1, s2) for _, rows in TPD.ROWS for _, s1, s2, _, _ in rows} == want
    # the copies: set on every stage but a request's last, the third one S rows behind the second
    assert any(xo3 == 0 for _, rows in TPD.ROWS for *_, xo3 in rows) and any(xo3 for _, rows in TPD.ROWS for *_, xo3 in rows)
    NET_CALLS.clear()
    for j, (_, kw, b) in enumerate(REQS):
        s, scale2, nested = used[j]
        alone = _solver(dtype, s, scale2, nested, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, used[j])
    # (the second condition guides: the same request under plain classifier-free guidance of its scale ends elsewhere)
    base = _solver(dtype, used[0][0] if used[0][0] != 1.0 else 3.0, pair=False, cond=conds[0][0], uncond=conds[0][1])
    assert not torch.equal(got[0], base.sample(xs[0], **REQS[0][1]))


def test_steady_tick_is_one_network_call_one_run_and_one_copy(doubles):
    dpm = _solver()
    g = torch.Generator().manual_seed(1)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 8, 8, generator=g) for j in range(10)]
    pool = dpm.request_pool(slots=40, pair=True)
    hs = [pool.submit(x, steps=8, order=2) for x in xs]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        nets = len(NET_CALLS)
        done.update(pool.step())
        assert NET_CALLS[nets:] == [120]
    assert pool.copies == 6 and TPD.CALLS[-2:] == [(20, FILL_P), (20, LAUNCH_P)]
    runs, rows = TPD.ROWS[-1]
    assert runs == 1 and len({r[0] for r in rows}) == 20                           # ONE run: one launch
    x_out = {int(pool._x[k].data_ptr()) for k in (0, 1)}
    for x, _, _, gptr, xo3 in rows:                                                # the third copy: 2S rows behind x_out
        assert any(xo3 - 2 * 40 * pool._rowb - base in range(0, 40 * pool._rowb, pool._rowb) for base in x_out)
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 40 * (L.TABLE_ROW_BYTES + L.TABLE_PAIR_BYTES) + 15) // 16 * 16
    assert pool._tabb == (L.table_bytes(40, L.TABLE_PAIR) + 15) // 16 * 16 and pool._nS == 120
    while pool:
        done.update(pool.step())
    for h, x in zip(hs, xs):
        assert torch.equal(done[h], dpm.sample(x, steps=8, order=2))


def test_the_tick_writes_what_the_planner_and_the_binder_write():
    """the two scales over the wrapper's record = the record sample() builds for a wrapper of those scales"""
    x = torch.randn(1, 4, 8, 8)
    ref, base = _solver(s=7.5, scale2=9.0, nested=True), _solver()
    a = ref._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
    b = base._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
    pool = base.request_pool(slots=2, pair=True)
    s1, s2 = pool._pair_params(7.5, (9.0, True), None)
    for sa, sb in zip(a.stages, b.stages):
        sa, sb = ref._prep_stage(sa.copy()), base._prep_stage(sb.copy())
        assert sb.guidance == L.GUIDE["classifier-free-2"]
        sb.cfg_scale, sb.cg_scale = np.float32(s1), np.float32(s2)
        assert bytes(sa) == bytes(sb)


# ---- refusals, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if any device
# work preceded them
def _raises(exc, text):
    """the FULL message"""
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    dpm, plain = _solver(), _solver(pair=False)
    with _raises(ValueError, "request_pool: pair=True belongs to a slab pool (slots=...)"):
        dpm.request_pool(pair=True)
    needs = ("request_pool: pair=True needs a cfg_pair wrapper (guidance over two conditions with a second scale other than 0)")
    for other in (plain, _solver(scale2=0.0), D.DPM_Solver(D.model_wrapper(_net, make_schedule("sd")), make_schedule("sd"))):
        with _raises(ValueError, needs):
            other.request_pool(slots=8, pair=True)
    for name, why in (("sde", "no noise epilogue"), ("thresholding", "no thresholding"), ("inpaint", "no mask-blend epilogue"),
                      ("rescale", "no guidance rescale"), ("apg", "no projected guidance"),
                      ("zero_star", "no CFG-Zero* projection")):
        with _raises(NotImplementedError, "request_pool: pair=True with %s=True -- the two-condition kernel has %s (a follow-up)"
                                          % (name, why)):
            dpm.request_pool(slots=8, pair=True, **{name: True})
    # without the switch: the refusal every pool gave, its tail naming the switch now
    P = r"^guidance over two conditions \(cfg_pair\): request_pool"
    for kw in ({}, dict(slots=8), dict(slots=8, sde=True)):
        with pytest.raises(NotImplementedError, match=P + r".*request_pool\(slots=\.\.\., pair=True\)"):
            dpm.request_pool(**kw)
    pool = dpm.request_pool(slots=8, pair=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError, match=r"^guidance over two conditions \(cfg_pair\): sample_unipc"):
        pool.submit_unipc(x, steps=6)
    with _raises(NotImplementedError, "slab pool: sde=True -- SDE stages have no table kernel; use request_pool() without slots"):
        pool.submit(x, steps=6, sde=True, seed=3)
    with _raises(NotImplementedError, "slab pool: blend= -- mask-blend stages take the table in a pool built with "
                                      "request_pool(slots=..., inpaint=True) only"):
        pool.submit(x, steps=6, blend=object())
    with _raises(NotImplementedError, "slab pool: pair= -- two-condition stages take the table in a pool built with "
                                      "request_pool(slots=..., pair=True) only"):
        plain.request_pool(slots=8).submit(x, steps=6, pair=(1.5, False))
    with _raises(ValueError, "slab pool: condition2= belongs to a pool built with request_pool(slots=..., pair=True)"):
        plain.request_pool(slots=8).submit(x, steps=6, condition2=torch.ones(1, 1))
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, method="singlestep")
    # the arguments' own checks: cfg_pair's, with its texts
    with _raises(ValueError, "slab pool: guidance_scale= in a pair=True pool needs pair=(scale2, nested) -- the wrapper does not "
                             "keep `nested`, so the second scale's meaning would be a guess"):
        pool.submit(x, steps=6, guidance_scale=2.0)
    for bad in (1.5, (1.5,), (1.5, False, 0), "ab"):
        with _raises(ValueError, "slab pool: pair= takes (scale2, nested), got %r" % (bad,)):
            pool.submit(x, steps=6, pair=bad)
    for bad in (True, "2", float("inf"), float("nan"), None):
        with _raises(ValueError, "cfg_pair: scale2 must be a finite real number, got %r" % (bad,)):
            pool.submit(x, steps=6, pair=(bad, False))
    for bad in (1, 0, "True", None):
        with _raises(ValueError, "cfg_pair: nested must be a bool, got %r" % (bad,)):
            pool.submit(x, steps=6, pair=(1.5, bad))
    for bad in (True, "2", float("inf")):
        with _raises(ValueError, "cfg_pair: the wrapper's guidance_scale must be a finite real number, got %r" % (bad,)):
            pool.submit(x, steps=6, guidance_scale=bad, pair=(1.5, False))
    # a second scale of 0 is plain two-branch guidance: no row of a [3S] slab
    for kw in (dict(pair=(0.0, False)), dict(guidance_scale=2.5, pair=(2.5, True)), dict(pair=(3.0, True))):
        with pytest.raises(NotImplementedError, match="the second scale comes out 0, which is plain two-branch guidance.*"
                                                      "half noise networks.*cannot reproduce those bits"):
            pool.submit(x, steps=6, **kw)
    # the other kinds' arguments belong to a classifier-free wrapper
    with pytest.raises(ValueError, match="guidance_rescale belong to a classifier-free wrapper"):
        pool.submit(x, steps=6, guidance_rescale=0.5)
    with pytest.raises(ValueError, match="apg= belongs to a classifier-free wrapper"):
        pool.submit(x, steps=6, apg=(0.5, 0.0, 0.0))
    with pytest.raises(ValueError, match="zero_star= belongs to a classifier-free wrapper"):
        pool.submit(x, steps=6, zero_star=True)
    # the sample has to be a row of the table pair kernel: refused at the first submit
    for shape, per in (((2, 1, 2, 2), 4), ((2, 3, 2, 2), 12), ((1, 3, 5, 7), 105)):
        with _raises(NotImplementedError, "slab pool: pair=True with a sample of %d elements -- a two-condition row of the table "
                                          "is whole 8-element groups of 16-byte aligned buffers; use request_pool() without "
                                          "slots" % per):
            dpm.request_pool(slots=8, pair=True).submit(torch.randn(*shape), steps=6)
    # ... which a well-formed request on the host then meets
    for kw in ({}, dict(guidance_scale=1.0, pair=(2.0, True)), dict(pair=(0.5, False), condition2=torch.ones(2, 1))):
        with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
            dpm.request_pool(slots=8, pair=True).submit(x, steps=6, **kw)
    assert not pool and pool.step() == {}
