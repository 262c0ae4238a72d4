"""A slab pool that holds EVERY kind of request at once (DPM_Solver.request_pool(slots=12, sde=True, inpaint=True)) without a GPU:
the churn scenario of tests/mixed_pool_cases.py on the numpy doubles of tests/table_blend_double.py.  36 plain, UniPC, SDE and
inpainting requests through 12 rows: rows change kind as they are freed and handed on, the lowest active row -- whose options
are the call's, seed included -- is of every kind in turn, and every result must be the bits of the request run alone.  Every
tick is one network call and one FILL / LAUNCH pair that carries DPM_TABLE_NOISE | DPM_TABLE_BLEND.  The same in small for a
thresholding pool built with sde=True: DPM_TABLE_NOISE | DPM_TABLE_THRESH."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import mixed_pool_cases as M
import table_blend_double as TBD
import table_thresh_double as TTD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pool_host import NET_CALLS, _net

BOTH = L.TABLE_NOISE | L.TABLE_BLEND
NS = make_schedule("sd")


def _solver(cfg, dtype, cond=None, uncond=None, cxt=None, thresholding=False):
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_net, NS, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_net, NS)
    return D.DPM_Solver(fn, NS, algorithm_type="dpmsolver++", correcting_xt_fn=cxt,
                        correcting_x0_fn="dynamic_thresholding" if thresholding else None, **kw)


def test_the_scenario_hands_every_kind_of_row_to_every_kind():
    """properties of the scenario table, by the restated admission rule (the tests that run it check the restatement)"""
    sps = M.specs()
    ticks, admitted = M.simulate(sps)
    assert len(sps) == 36 and {sp["kind"] for sp in sps} == set(M.KINDS) and max(sp["tick"] for sp in sps) + 1 == 9
    assert sum(sp["b"] * M.n_stages(sp) for sp in sps) > 12 * 30             # they cannot all fit: the pool churns
    assert M.handovers(sps, ticks) == {(a, b) for a in M.KINDS for b in M.KINDS}
    assert {sps[occ[min(occ)]]["kind"] for occ in ticks if occ} == set(M.KINDS)      # the lowest active row: every kind
    assert len(M.all_kind_ticks(sps, ticks)) >= 2 and len(M.counting_ticks(sps, ticks, admitted)) == 2
    assert max(admitted[sp["j"]] - sp["tick"] for sp in sps) >= 2             # the FIFO is exercised
    # what the requests rotate over
    assert {sp["b"] for sp in sps} == {1, 3} and {sp["kw"]["steps"] for sp in sps} == set(range(4, 10))
    for kind, orders in (("plain", {1, 2, 3}), ("blend", {1, 2, 3}), ("unipc", {1, 2}), ("sde", {1, 2})):
        mine = [sp for sp in sps if sp["kind"] == kind]
        assert {sp["kw"]["order"] for sp in mine} == orders, kind
        assert {sp["kw"]["denoise_to_zero"] for sp in mine} == {False, True}, kind
        assert {sp["b"] for sp in mine} == {1, 3}, kind
    assert {(sp["kw"]["variant"], sp["kw"]["order"]) for sp in sps if sp["kind"] == "unipc"} == \
        {(v, o) for v in ("bh1", "bh2") for o in (1, 2)}
    seeds = {sp["kw"]["seed"] for sp in sps if sp["kind"] == "sde"}
    assert 0 in seeds and any(s >= 1 << 63 for s in seeds) and len(seeds) >= 4
    assert {(sp["mode"], sp["full_mask"]) for sp in sps if sp["kind"] == "blend"} == \
        {(m, f) for m in ("x0", "intermediates") for f in (False, True)}
    # the thresholding pool in small: 10 requests of 18 rows in 8
    thr = M.thresh_specs()
    _, admitted = M.simulate(thr, M.THR_SLOTS)
    assert len(thr) == 10 and max(admitted[sp["j"]] - sp["tick"] for sp in thr) >= 2


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_churning_pool_of_every_kind_equals_every_request_alone(monkeypatch, dtype, cfg):
    TBD.install_table_blend_sde_double(monkeypatch, S, D)
    NET_CALLS.clear()
    sps = M.specs()
    xs, conds, mbs = M.tensors(sps, dtype, "cpu", NS, D.MaskBlend)
    pool = _solver(cfg, dtype).request_pool(slots=M.SLOTS, sde=True, inpaint=True)
    assert isinstance(pool, SlabPool)
    seen = {"nets": 0, "calls": 0, "runs": 0}

    def each_tick(tick, occ, info):
        assert occ, tick                                                        # (no idle tick in this scenario)
        assert NET_CALLS[seen["nets"]:] == [2 * M.SLOTS if cfg else M.SLOTS], tick      # ONE network call, on the whole slab
        R = len(occ)
        assert TBD.CALLS[seen["calls"]:] == [(R, L.TABLE_FILL | BOTH), (R, L.TABLE_LAUNCH | BOTH)], tick
        # the runs the library counted into the table's header: what the restated grouping rule expects of this tick
        e = info["expect"]
        assert len(TBD.RUNS) == seen["runs"] + 1 and TBD.RUNS[-1][0] == e["noise"] + e["blend"] + e["table"] + e["table_unipc"], tick
        assert info["copies"] == 1 or (info["admitted"] and info["copies"] == 2), (tick, info)     # a steady tick: one copy
        seen["nets"], seen["calls"], seen["runs"] = len(NET_CALLS), len(TBD.CALLS), len(TBD.RUNS)
    got, ticks = M.run(pool, sps, xs, conds, mbs, cfg, each_tick)
    assert ticks == M.simulate(sps)[0], "mixed_pool_cases.simulate is not the pool's admission rule"
    assert sorted(got) == list(range(len(sps)))
    assert not pool._blends and not pool._ropts, "the pool keeps nothing of a finished request"
    assert any(runs >= 2 and nb > 0 for runs, nb, _ in TBD.RUNS) and TBD.BLENDS
    NET_CALLS.clear()
    for sp in sps:
        j = sp["j"]
        want = M.alone(lambda c, u, cxt: _solver(cfg, dtype, c, u, cxt), sp, xs[j], conds[j], mbs[j], cfg)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, sp
        assert torch.equal(got[j], want), sp


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_thresholding_pool_built_with_sde_runs_its_rows_under_both_flags(monkeypatch, dtype, cfg):
    TTD.install_table_thresh_double(monkeypatch, S, D)
    NET_CALLS.clear()
    flags = L.TABLE_NOISE | L.TABLE_THRESH
    sps = M.thresh_specs()
    xs, conds, mbs = M.tensors(sps, dtype, "cpu", NS, D.MaskBlend, shape=M.THR_SHAPE)
    dpm = _solver(cfg, dtype, thresholding=True)
    pool = dpm.request_pool(slots=M.THR_SLOTS, thresholding=True, sde=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError):                                    # its SDE submit stays refused
        pool.submit(xs[0], steps=6, sde=True, seed=1)
    seen = {"nets": 0, "calls": 0, "rows": 0}

    def each_tick(tick, occ, info):
        assert NET_CALLS[seen["nets"]:] == [2 * M.THR_SLOTS if cfg else M.THR_SLOTS], tick
        R = len(occ)
        assert TTD.CALLS[seen["calls"]:] == [(R, L.TABLE_FILL | flags), (R, L.TABLE_LAUNCH | flags)], tick
        runs, xptrs = TTD.ROWS[seen["rows"]]
        assert len(TTD.ROWS) == seen["rows"] + 1 and runs == 1 and len(set(xptrs)) == R and 0 not in xptrs, tick
        seen["nets"], seen["calls"], seen["rows"] = len(NET_CALLS), len(TTD.CALLS), len(TTD.ROWS)
    got, ticks = M.run(pool, sps, xs, conds, mbs, cfg, each_tick)
    assert ticks == M.simulate(sps, M.THR_SLOTS)[0]
    assert sorted(got) == list(range(len(sps))) and not pool._ropts
    assert pool._tabb == (L.table_bytes(M.THR_SLOTS, flags) + 15) // 16 * 16
    NET_CALLS.clear()
    for sp in sps:
        j = sp["j"]
        want = M.alone(lambda c, u, cxt: _solver(cfg, dtype, c, u, thresholding=True), sp, xs[j], conds[j], None, cfg)
        assert got[j].dtype == want.dtype and torch.equal(got[j], want), sp
    plain = M.alone(lambda c, u, cxt: _solver(cfg, dtype, c, u), sps[0], xs[0], conds[0], None, cfg)
    assert not torch.equal(got[0], plain)                                        # (the thresholding is there)
