"""A Perp-Neg slab pool (DPM_Solver.request_pool(slots=S, perp_neg=True)) without a GPU: the host code on the numpy doubles of
tests/table_perp_double.py -- DPM_TABLE_FILL | DPM_TABLE_PERP by the real library, the per-row doubles at LAUNCH
(perp_double.stage, then the two copies).  A staggered pool: 8 rows, 12 requests of 1 and 3 samples, steps 4..9, orders 1..3 (the
schedule of tests/test_slab_pair_host.py), so that requests wait and rows are reused; every request brings its own three
conditions, guidance scale and negative scale; every result must be the bits of sample() on the request alone, on a solver whose
wrapper is cfg_perp_neg(model_wrapper(..., guidance_scale=s, condition=c, unconditional_condition=u), n, w)."""
import re

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_perp_double as TPP
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pair_host import REQS, SLOTS

FILL_P, LAUNCH_P = L.TABLE_FILL | L.TABLE_PERP, L.TABLE_LAUNCH | L.TABLE_PERP
NET_CALLS = []
# request j's own (s, w): guidance scale 1.0 and a negative w among them
OWN = [((1.0, 1.5, 3.0, 7.5)[j % 4], (0.75, 2.5, -1.25)[j % 3]) for j in range(12)]


def _net(x, t, c):
    """elementwise in the row -- its state, its time, its condition -- in exactly rounded operations only (the same bits whatever
    the batch), and not linear in the condition: the negative direction is neither parallel nor perpendicular to the positive one"""
    NET_CALLS.append(int(x.shape[0]))
    xf = x.float()
    xc = torch.clamp(xf, -2.0, 2.0)
    cc = c.float().repeat_interleave(x.shape[0] // c.shape[0], dim=0).reshape(-1, 1, 1, 1)
    out = xf * (0.5 + 0.1 * cc) + 0.1 * xc * xc * cc * cc + 0.05 * cc + 0.0001 * t.float().reshape(-1, 1, 1, 1)
    return out.to(x.dtype)


@pytest.fixture
def doubles(monkeypatch):
    TPP.install_table_perp_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _solver(dtype=torch.float32, s=3.0, w=1.5, cond=None, uncond=None, neg=None, kind="perp", **skw):
    ns = make_schedule("sd")
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    kw.update(skw)
    kw.setdefault("algorithm_type", "dpmsolver++")
    fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=s,
                         condition=torch.ones(1, 1) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    neg = torch.full((1, 1), 0.5) if neg is None else neg
    if kind == "perp":
        fn = D.cfg_perp_neg(fn, neg, w)
    elif kind == "pair":
        fn = D.cfg_pair(fn, neg, w)
    return D.DPM_Solver(fn, ns, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_perp_slab_pool_equals_every_request_alone(doubles, dtype):
    g = torch.Generator().manual_seed(221)
    xs = [(2.0 * torch.randn(b, 4, 8, 8, generator=g)).to(dtype) for _, _, b in REQS]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0,
              torch.rand(b if j % 4 == 2 else 1, 1, generator=g) + 0.5) for j, (_, _, b) in enumerate(REQS)]
    dpm = _solver(dtype)
    pool = dpm.request_pool(slots=SLOTS, perp_neg=True)
    assert isinstance(pool, SlabPool)
    assert {b for _, _, b in REQS} == {1, 3} and {kw["steps"] for _, kw, _ in REQS} == set(range(4, 10))
    assert {kw["order"] for _, kw, _ in REQS} == {1, 2, 3} and sum(kw["denoise_to_zero"] for _, kw, _ in REQS) == 1
    assert any(s == 1.0 for s, _ in OWN) and any(w < 0 for _, w in OWN)
    handles, got, rows_of, admitted_at, tick, used = {}, {}, {}, {}, 0, {}
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kw, b) in enumerate(REQS):
            if t == tick:
                s, w = OWN[j]
                okw = dict(guidance_scale=s, neg_scale=w)
                if j == 3:
                    del okw["guidance_scale"]                    # the wrapper's guidance scale, the request's negative scale
                    s = 3.0
                if j == 5:
                    del okw["neg_scale"]                         # the request's guidance scale, the wrapper's negative scale
                    w = 1.5
                if j == 7:
                    okw = {}                                     # both the wrapper's
                    s, w = 3.0, 1.5
                used[j] = (s, w)
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1],
                                    negative_condition=conds[j][2], **kw, **okw)] = j
        nets, calls, launches = len(NET_CALLS), len(TPP.CALLS), len(TPP.ROWS)
        done = pool.step()
        for h, (rws, _) in pool._rows.items():
            if handles[h] not in rows_of:
                rows_of[handles[h]], admitted_at[handles[h]] = list(rws), tick
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [3 * SLOTS]               # ONE network call per tick, on the whole [3S] slab
            R = TPP.CALLS[calls][0]
            assert TPP.CALLS[calls:] == [(R, FILL_P), (R, LAUNCH_P)]
            assert len(TPP.ROWS) == launches + 1
            runs, rows = TPP.ROWS[-1]
            # every active row is a Perp-Neg row; a group agrees on n, batch (1 here: a row is a sample) and DPM_F_TO_X0
            assert len(rows) == R and 1 <= runs <= 2
        else:
            assert TPP.CALLS[calls:] == []
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(REQS)))
    assert any(admitted_at[j] > REQS[j][0] for j in admitted_at), admitted_at      # requests waited for rows ...
    first = {}
    reused = [j for j in sorted(rows_of, key=lambda j: admitted_at[j]) for r in rows_of[j] if first.setdefault(r, j) != j]
    assert reused, rows_of                                                         # ... and rows were reused
    # the table carried every request's own two scales
    want = {(float(np.float32(s)), float(np.float32(w))) for s, w in used.values()}
    assert {(s, w) for _, rows in TPP.ROWS for _, s, w, _, _ in rows} == want
    # the copies: set on every stage but a request's last, the third one S rows behind the second
    assert any(xo3 == 0 for _, rows in TPP.ROWS for *_, xo3 in rows) and any(xo3 for _, rows in TPP.ROWS for *_, xo3 in rows)
    NET_CALLS.clear()
    for j, (_, kw, b) in enumerate(REQS):
        s, w = used[j]
        alone = _solver(dtype, s, w, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, used[j])
    # (the projection guides: the same request under cfg_pair's linear blend of the same two scales ends elsewhere)
    lin = _solver(dtype, *used[0], *[c.expand(REQS[0][2], -1) for c in conds[0]], kind="pair")
    assert not torch.equal(got[0], lin.sample(xs[0], **REQS[0][1]))


def test_steady_tick_is_one_network_call_one_run_and_one_copy(doubles):
    dpm = _solver()
    g = torch.Generator().manual_seed(1)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 8, 8, generator=g) for j in range(10)]
    pool = dpm.request_pool(slots=40, perp_neg=True)
    hs = [pool.submit(x, steps=8, order=2) for x in xs]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector
    assert pool.copies == 2
    for _ in range(4):
        nets = len(NET_CALLS)
        done.update(pool.step())
        assert NET_CALLS[nets:] == [120]
    assert pool.copies == 6 and TPP.CALLS[-2:] == [(20, FILL_P), (20, LAUNCH_P)]
    runs, rows = TPP.ROWS[-1]
    assert runs == 1 and len({r[0] for r in rows}) == 20                           # ONE run: one launch
    x_out = {int(pool._x[k].data_ptr()) for k in (0, 1)}
    for x, _, _, gptr, xo3 in rows:                                                # the third copy: 2S rows behind x_out
        assert any(xo3 - 2 * 40 * pool._rowb - base in range(0, 40 * pool._rowb, pool._rowb) for base in x_out)
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 40 * (L.TABLE_ROW_BYTES + L.TABLE_PAIR_BYTES) + 15) // 16 * 16
    assert pool._tabb == (L.table_bytes(40, L.TABLE_PERP) + 15) // 16 * 16 and pool._nS == 120
    while pool:
        done.update(pool.step())
    for h, x in zip(hs, xs):
        assert torch.equal(done[h], dpm.sample(x, steps=8, order=2))


def test_the_tick_writes_what_the_planner_and_the_binder_write():
    """the two scales over the wrapper's record = the record sample() builds for a wrapper of those scales, flag included"""
    x = torch.randn(1, 4, 8, 8)
    ref, base = _solver(s=7.5, w=-0.25), _solver()
    a = ref._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
    b = base._sample_plan(x, 5, 1e-3, 1.0, 2, "time_uniform", "multistep", True, True, "dpmsolver")
    pool = base.request_pool(slots=2, perp_neg=True)
    s, w = pool._perp_params(7.5, -0.25, None, None, None)
    for sa, sb in zip(a.stages, b.stages):
        sa, sb = ref._prep_stage(sa.copy()), base._prep_stage(sb.copy())
        assert sb.guidance == L.GUIDE["classifier-free-2"] and sb.flags & L.F_CFG2_PERP
        sb.cfg_scale, sb.cg_scale = np.float32(s), np.float32(w)
        assert bytes(sa) == bytes(sb)
    assert pool._perp_params(None, 2.0, None, None, None) == (3.0, 2.0)            # either scale without the other
    assert pool._perp_params(2.0, None, None, None, None) == (2.0, 1.5)
    assert pool._perp_params(None, None, torch.ones(1, 1), None, None) is None


def test_the_negative_condition_is_checked_like_the_other_two(doubles):
    pool = _solver().request_pool(slots=8, perp_neg=True)
    x = torch.randn(2, 4, 8, 8)
    with pytest.raises(ValueError, match="slab pool: negative_condition must be a tensor of leading dimension 2 or 1"):
        pool.submit(x, steps=6, negative_condition=torch.ones(3, 1))
    with pytest.raises(ValueError, match="slab pool: condition and negative_condition differ in shape or dtype"):
        pool.submit(x, steps=6, negative_condition=torch.ones(2, 2))
    assert not pool


# ---- refusals, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if any device
# work preceded them
def _raises(exc, text):
    """the FULL message"""
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, 4, 8, 8)
    dpm, plain, pair = _solver(), _solver(kind="cfg"), _solver(kind="pair")
    with _raises(ValueError, "request_pool: perp_neg=True belongs to a slab pool (slots=...)"):
        dpm.request_pool(perp_neg=True)
    needs = "request_pool: perp_neg=True needs a cfg_perp_neg wrapper (Perp-Neg guidance with a negative scale other than 0)"
    for other in (plain, pair, _solver(w=0.0), D.DPM_Solver(D.model_wrapper(_net, make_schedule("sd")), make_schedule("sd"))):
        with _raises(ValueError, needs):
            other.request_pool(slots=8, perp_neg=True)
    for name, why in (("sde", "no noise epilogue"), ("thresholding", "no thresholding"), ("inpaint", "no mask-blend epilogue"),
                      ("rescale", "no guidance rescale"), ("apg", "no projected guidance"),
                      ("zero_star", "no CFG-Zero* projection"), ("pair", "no linear second blend")):
        with _raises(NotImplementedError, "request_pool: perp_neg=True with %s=True -- the Perp-Neg kernel has %s (a follow-up)"
                                          % (name, why)):
            dpm.request_pool(slots=8, perp_neg=True, **{name: True})
    # without the switch: the refusals every pool gave, unchanged
    with _raises(NotImplementedError, "request_pool: pair=True with a cfg_perp_neg wrapper -- the table's two-condition rows "
                                      "have no per-sample pass (a follow-up)"):
        dpm.request_pool(slots=8, pair=True)
    P = r"^guidance over two conditions \(cfg_pair\): request_pool"
    for kw in (dict(slots=8), dict(slots=8, sde=True)):
        with pytest.raises(NotImplementedError, match=P):
            dpm.request_pool(**kw)
    pool = dpm.request_pool(slots=8, perp_neg=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError, match=r"^guidance over two conditions \(cfg_pair\): sample_unipc"):
        pool.submit_unipc(x, steps=6)
    with _raises(NotImplementedError, "slab pool: sde=True -- SDE stages have no table kernel; use request_pool() without slots"):
        pool.submit(x, steps=6, sde=True, seed=3)
    with _raises(NotImplementedError, "slab pool: blend= -- mask-blend stages take the table in a pool built with "
                                      "request_pool(slots=..., inpaint=True) only"):
        pool.submit(x, steps=6, blend=object())
    for name, v in (("neg_scale", 1.5), ("negative_condition", torch.ones(1, 1))):
        for other in (plain.request_pool(slots=8), pair.request_pool(slots=8, pair=True)):
            with _raises(NotImplementedError, "slab pool: %s= -- Perp-Neg stages take the table in a pool built with "
                                              "request_pool(slots=..., perp_neg=True) only" % name):
                other.submit(x, steps=6, **{name: v})
    for name, v in (("pair", (1.5, False)), ("condition2", torch.ones(1, 1))):
        with _raises(NotImplementedError, "slab pool: %s= in a perp_neg=True pool -- the Perp-Neg kernel takes one negative "
                                          "condition (negative_condition=, neg_scale=) and no second blend" % name):
            pool.submit(x, steps=6, **{name: v})
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, method="singlestep")
    # the arguments' own checks: cfg_perp_neg's, with its texts
    for bad in (True, "2", float("inf"), float("nan")):
        with _raises(ValueError, "cfg_perp_neg: neg_scale must be a finite real number, got %r" % (bad,)):
            pool.submit(x, steps=6, neg_scale=bad)
    for bad in (True, "2", float("inf")):
        with _raises(ValueError, "cfg_perp_neg: the wrapper's guidance_scale must be a finite real number, got %r" % (bad,)):
            pool.submit(x, steps=6, guidance_scale=bad)
    # a negative scale of 0 is plain two-branch guidance: no row of a [3S] slab
    for kw in (dict(neg_scale=0.0), dict(guidance_scale=2.5, neg_scale=-0.0), dict(neg_scale=0)):
        with pytest.raises(NotImplementedError, match="a negative scale of 0 is plain two-branch guidance.*"
                                                      "half noise networks.*cannot reproduce those bits"):
            pool.submit(x, steps=6, **kw)
    # the other kinds' arguments belong to a classifier-free wrapper
    with pytest.raises(ValueError, match="guidance_rescale belong to a classifier-free wrapper"):
        pool.submit(x, steps=6, guidance_rescale=0.5)
    with pytest.raises(ValueError, match="apg= belongs to a classifier-free wrapper"):
        pool.submit(x, steps=6, apg=(0.5, 0.0, 0.0))
    with pytest.raises(ValueError, match="zero_star= belongs to a classifier-free wrapper"):
        pool.submit(x, steps=6, zero_star=True)
    # the sample has to be a row of the table Perp-Neg kernel: refused at the first submit
    for shape, per in (((2, 1, 2, 2), 4), ((2, 3, 2, 2), 12), ((1, 3, 5, 7), 105)):
        with _raises(NotImplementedError, "slab pool: perp_neg=True with a sample of %d elements -- a Perp-Neg row of the table "
                                          "is whole 8-element groups of 16-byte aligned buffers; use request_pool() without "
                                          "slots" % per):
            dpm.request_pool(slots=8, perp_neg=True).submit(torch.randn(*shape), steps=6)
    # ... which a well-formed request on the host then meets
    for kw in ({}, dict(guidance_scale=1.0), dict(neg_scale=0.5, negative_condition=torch.ones(2, 1))):
        with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
            dpm.request_pool(slots=8, perp_neg=True).submit(x, steps=6, **kw)
    assert not pool and pool.step() == {}
