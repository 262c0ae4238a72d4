"""The slab pool's staging ring (dpm_solver_amd/slab.py, _RING pinned slots, each guarded by the event behind its table copy)
under a strict model of the copy stream -- tests/staging_double.py: the device is arbitrarily slow, a copy has happened only
once the host has waited on an event recorded at or after it, and until then its pinned source must not change -- without a GPU.

One churn scenario per flavour of slab pool, each on that flavour's own host helpers and numpy doubles: the mixed pool of
tests/mixed_pool_cases.py (sde=True, inpaint=True), its thresholding pool (thresh_specs), and rescale=True, apg=True,
zero_star=True, pair=True, perp_neg=True on the staggered requests of their host tests.  The staggered requests of
tests/test_slab_thresh_host.py admit on one tick only once the ring has wrapped, so three late requests (LATE) follow them.

Every scenario runs at least 3 * _RING ticks and admits on at least two ticks at or after tick _RING, by the pool's admission
rule restated in mixed_pool_cases.simulate: a slot's `t_cur` range -- the second, small copy of an admitting tick, whose own
event the pool drops -- is rewritten while an earlier copy of it is still on record.  Checked:

  * no pending copy's source is ever rewritten, for every flavour;
  * the results are the bits of the same scenario on the flavour's doubles alone: the model changes nothing;
  * every wait the pool makes is on the table copy of the slot it is about to refill -- the tick _RING ticks back -- and on no
    younger one: the host may stay _RING - 1 ticks ahead, the ring does not quietly serialise;
  * every tensor step() returned is unchanged when the pool has drained (fresh tensors, not views of a slab row);
  * the model catches what it is for: a pool whose waits pass nothing is caught at tick _RING on slot 0, and a pool that keeps
    the event of the copy before the table's is caught too.  Both mutants are monkeypatches of this file, on the CPU only."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import mixed_pool_cases as M
import staging_double as SD
import table_apg_double as TAD
import table_blend_double as TBD
import table_pair_double as TPD
import table_perp_double as TPP
import table_rescale_double as TRD
import table_thresh_double as TTD
import table_zstar_double as TZD
import test_slab_apg_host as APG
import test_slab_mixed_host as MIX
import test_slab_pair_host as PAIR
import test_slab_perp_host as PERP
import test_slab_rescale_host as RSC
import test_slab_zstar_host as ZST
from dpm_solver_amd.slab import _RING, SlabPool
from test_slab_thresh_host import REQS

# (tick of submission, kwargs, b) behind test_slab_thresh_host.REQS: requests admitted once the ring has wrapped
LATE = [(6, dict(steps=5, order=2), 3), (9, dict(steps=4, order=3, denoise_to_zero=True), 1), (10, dict(steps=6, order=1), 3)]


class Scenario:
    """one flavour: `install` its doubles, `pool` a fresh pool, `sps` the requests as mixed_pool_cases.simulate takes them
    (j, tick, b, kw with steps and denoise_to_zero), `submit(pool, j)` request j"""

    def __init__(self, install, slots, sps, pool, submit):
        self.install, self.slots, self.sps, self.pool, self.submit = install, slots, sps, pool, submit


def _sps(reqs):
    return [dict(j=j, tick=t, b=b, kw=dict(kw, denoise_to_zero=kw.get("denoise_to_zero", False))) for j, (t, kw, b) in enumerate(reqs)]


def _tensors(reqs, seed, dtype, third=False):
    """x_T and per-request conditions as the flavours' host tests draw them"""
    g = torch.Generator().manual_seed(seed)
    xs = [(2.0 * torch.randn(b, 4, 8, 8, generator=g)).to(dtype) for _, _, b in reqs]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             + ((torch.rand(b if j % 4 == 2 else 1, 1, generator=g) + 0.5,) if third else ()) for j, (_, _, b) in enumerate(reqs)]
    return xs, conds


def _mixed():
    dtype, cfg = torch.float16, True
    sps = M.specs()
    xs, conds, mbs = M.tensors(sps, dtype, "cpu", MIX.NS, D.MaskBlend)
    return Scenario(TBD.install_table_blend_sde_double, M.SLOTS, sps,
                    lambda: MIX._solver(cfg, dtype).request_pool(slots=M.SLOTS, sde=True, inpaint=True),
                    lambda pool, j: M.submit(pool, sps[j], xs[j], conds[j], mbs[j], cfg))


def _thresh():
    dtype, cfg = torch.float32, True
    sps = M.thresh_specs()
    xs, conds, mbs = M.tensors(sps, dtype, "cpu", MIX.NS, D.MaskBlend, shape=M.THR_SHAPE)
    return Scenario(TTD.install_table_thresh_double, M.THR_SLOTS, sps,
                    lambda: MIX._solver(cfg, dtype, thresholding=True).request_pool(slots=M.THR_SLOTS, thresholding=True, sde=True),
                    lambda pool, j: M.submit(pool, sps[j], xs[j], conds[j], None, cfg))


def _staggered(install, seed, pool, own, dtype=torch.float32):
    """rescale / apg / zero_star: REQS + LATE in ten rows, request j with `own(j)` keyword arguments"""
    reqs = REQS + LATE
    xs, conds = _tensors(reqs, seed, dtype)
    return Scenario(install, 10, _sps(reqs), lambda: pool(dtype),
                    lambda p, j: p.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], **reqs[j][1], **own(j)))


def _rescale():
    return _staggered(TRD.install_table_rescale_double, 213, lambda dt: RSC._solver(dt, 3.0, 0.5).request_pool(slots=10, rescale=True),
                      lambda j: dict(zip(("guidance_scale", "guidance_rescale"), RSC._guide(j))))


def _apg():
    return _staggered(TAD.install_table_apg_double, 215,
                      lambda dt: APG._solver(dt, 3.0, (0.5, 10.0, -0.25)).request_pool(slots=10, apg=True),
                      lambda j: dict(zip(("guidance_scale", "apg"), APG._own(j))))


def _zstar():
    return _staggered(TZD.install_table_zstar_double, 217, lambda dt: ZST._solver(dt, 3.0, True).request_pool(slots=10, zero_star=True),
                      lambda j: dict(zip(("guidance_scale", "zero_star"), ZST._own(j))))


def _three(install, seed, mod, flag, third, own):
    dtype = torch.float16
    xs, conds = _tensors(PAIR.REQS, seed, dtype, third=True)
    return Scenario(install, PAIR.SLOTS, _sps(PAIR.REQS), lambda: mod._solver(dtype).request_pool(slots=PAIR.SLOTS, **{flag: True}),
                    lambda p, j: p.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1],
                                          **{third: conds[j][2]}, **PAIR.REQS[j][1], **own(j)))


def _pair():
    return _three(TPD.install_table_pair_double, 219, PAIR, "pair", "condition2",
                  lambda j: dict(guidance_scale=PAIR.OWN[j][0], pair=PAIR.OWN[j][1:]))


def _perp():
    return _three(TPP.install_table_perp_double, 221, PERP, "perp_neg", "negative_condition",
                  lambda j: dict(zip(("guidance_scale", "neg_scale"), PERP.OWN[j])))


FLAVOURS = dict(mixed=_mixed, thresholding=_thresh, rescale=_rescale, apg=_apg, zero_star=_zstar, pair=_pair, perp_neg=_perp)


@pytest.fixture(params=sorted(FLAVOURS))
def scenario(request, monkeypatch):
    sc = FLAVOURS[request.param]()
    sc.install(monkeypatch, S, D)
    return sc


def drive(sc):
    """submit and step until the pool drains.  Returns ({j: result}, {j: its clone at retirement}, ticks run)"""
    pool = sc.pool()
    assert isinstance(pool, SlabPool)
    handles, got, snap, tick = {}, {}, {}, 0
    while tick <= max(sp["tick"] for sp in sc.sps) or pool:
        for sp in sc.sps:
            if sp["tick"] == tick:
                handles[sc.submit(pool, sp["j"])] = sp["j"]
        for h, out in pool.step().items():
            got[handles[h]], snap[handles[h]] = out, out.clone()
        tick += 1
    assert sorted(got) == list(range(len(sc.sps)))
    return got, snap, pool._tick


def test_every_scenario_wraps_the_ring_and_admits_behind_it():
    """from the scenarios, by the restated admission rule: at least 3 * _RING ticks, none of them idle, and requests admitted
    on at least two ticks at or after tick _RING (the drive below checks the restatement's tick count against the pool's)"""
    assert sorted(FLAVOURS) == sorted(["mixed", "thresholding", "rescale", "apg", "zero_star", "pair", "perp_neg"])
    for name, make in FLAVOURS.items():
        sc = make()
        ticks, admitted = M.simulate(sc.sps, sc.slots)
        assert len(ticks) >= 3 * _RING and all(ticks), (name, len(ticks))
        assert len({t for t in admitted.values() if t >= _RING}) >= 2, (name, sorted(set(admitted.values())))


def test_no_pending_copy_is_rewritten_and_nothing_else_changes(scenario, monkeypatch):
    sc = scenario
    ticks, admitted = M.simulate(sc.sps, sc.slots)
    want, _, n = drive(sc)                                  # the flavour's doubles alone
    assert n == len(ticks), "mixed_pool_cases.simulate is not the pool's admission rule"
    m = SD.install_staging_double(monkeypatch, S)
    got, snap, n = drive(sc)                                # staging_double.Torn: a pending copy's source was rewritten
    assert n == len(ticks) and m.checks > 6 * n and len(m.pins) == _RING
    # the model changes nothing: the bits of the doubles alone
    for j in want:
        assert got[j].dtype == want[j].dtype and torch.equal(got[j], want[j]), j
    # what step() returned is still what it was at retirement: fresh tensors, no view of a slab row later ticks overwrite
    for j in got:
        assert torch.equal(got[j], snap[j]), j
    # the copies: one table copy per tick from offset 0 of slot tick % _RING; on an admitting tick the time vector before it,
    # from the same slot
    admitting = set(admitted.values())
    tables = {}
    for tick, seq, slot, off, nbytes in m.copies:
        assert slot == tick % _RING, (tick, slot)
        if off == 0:
            assert tick not in tables
            tables[tick] = seq
        else:
            assert tick in admitting and tick not in tables, (tick, off)
    assert sorted(tables) == list(range(n)) and len(m.copies) == n + len(admitting)
    # the waits: one per tick, on the table copy of the slot it is about to refill and on no younger one
    assert [t for t, _ in m.waits] == list(range(n))
    for tick, seq in m.waits:
        assert seq == (tables[tick - _RING] if tick >= _RING else None), (tick, seq)
    # ... so at the end only the last _RING ticks' copies are still on record
    assert {p.tick for p in m.pending} == set(range(n - _RING, n))


def test_a_wait_that_passes_nothing_is_caught_on_slot_0_at_tick_RING(scenario, monkeypatch):
    """mutant 1 (CPU only): the pool's wait removed -- every _event_wait passes nothing"""
    m = SD.install_staging_double(monkeypatch, S)
    monkeypatch.setattr(S, "_event_wait", lambda ev: m.event_wait(None))
    with pytest.raises(SD.Torn, match="ring slot 0 ") as e:
        drive(scenario)
    assert e.value.tick == _RING and e.value.slot == 0 and e.value.issued == 0, str(e.value)


def test_the_event_of_the_copy_before_is_caught(scenario, monkeypatch):
    """mutant 2 (CPU only): _copy_to_device hands back the previous copy's event in place of its own -- the slot's event is
    then the one of its time vector's copy, or of the table copy one tick back"""
    m = SD.install_staging_double(monkeypatch, S)
    last = [None]

    def stale(dst, src):
        ev, last[0] = last[0], m.copy_to_device(dst, src)
        return ev
    monkeypatch.setattr(S, "_copy_to_device", stale)
    with pytest.raises(SD.Torn) as e:
        drive(scenario)
    assert e.value.tick == _RING and e.value.slot == 0, str(e.value)
