"""An inpainting slab pool (DPM_Solver.request_pool(slots=S, inpaint=True)) without a GPU: its host code on the numpy doubles of
tests/table_blend_double.py -- DPM_TABLE_FILL | DPM_TABLE_BLEND by the real library, the per-row doubles (KExt epilogue
included) at LAUNCH, kernel_double.blend behind dpm_blend_launch.  A staggered pool of about 30 requests, inpainting (both
MaskBlend modes, three mask shapes, a time_fn on some) and plain; every result must be the bits of sample() on the request
alone -- for an inpainting request, of a solver built with correcting_xt_fn=mb -- and every tick one network call."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_blend_double as TBD
from dpm_solver_amd import _lib as L
from dpm_solver_amd.slab import SlabPool
from engine_cases import make_schedule
from test_slab_pool_host import NET_CALLS, _net

FILL_B, LAUNCH_B = L.TABLE_FILL | L.TABLE_BLEND, L.TABLE_LAUNCH | L.TABLE_BLEND
SHAPE = (4, 8, 8)
NS = make_schedule("sd")


@pytest.fixture
def doubles(monkeypatch):
    TBD.install_table_blend_double(monkeypatch, S, D)
    NET_CALLS.clear()


def _solver(cfg, dtype, cond=None, uncond=None, cxt=None):
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_net, NS, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_net, NS)
    return D.DPM_Solver(fn, NS, algorithm_type="dpmsolver++", correcting_xt_fn=cxt, **kw)


def _time_fn(t):
    return 0.5 * t + 0.25


def _requests(n, dtype, seed=211):
    """(tick of submission, kwargs, b, MaskBlend or None): steps 4..9, orders 1..3, b in {1, 3}, denoise_to_zero on some; of
    every five requests one is plain, two re-noise a known image (x0 / noise) and two blend intermediates in (DiffEdit); masks
    [H,W], [1,C,H,W] and full size in rotation, a time_fn on every fourth"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for j in range(n):
        steps, b = 4 + j % 6, 1 + 2 * (j % 3 == 1)
        kw = dict(steps=steps, order=1 + (j // 2) % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 0],
                  denoise_to_zero=(j % 7 == 3))
        mshape = (SHAPE[1:], (1,) + SHAPE, (b,) + SHAPE)[j % 3]
        mask = (torch.rand(mshape, generator=g) > 0.5).to(dtype)
        if j % 5 == 0:
            mb = None
        elif j % 5 in (1, 3):
            mb = D.MaskBlend(NS, mask, x0=torch.randn((b,) + SHAPE, generator=g).to(dtype),
                             noise=torch.randn((b,) + SHAPE, generator=g).to(dtype), time_fn=_time_fn if j % 4 == 1 else None)
        else:
            mb = D.MaskBlend(NS, mask, intermediates=[torch.randn((b,) + SHAPE, generator=g).to(dtype) for _ in range(steps + 2)])
        out.append((j // 4, kw, b, mb))
    xs = [(2.0 * torch.randn((b,) + SHAPE, generator=g)).to(dtype) for _, _, b, _ in out]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b, _) in enumerate(out)]
    return out, xs, conds


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_inpainting_slab_pool_equals_every_request_alone(doubles, dtype, cfg):
    reqs, xs, conds = _requests(30, dtype)
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=40, inpaint=True)
    assert isinstance(pool, SlabPool)
    handles, got, tick = {}, {}, 0
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kw, b, mb) in enumerate(reqs):
            if t == tick:
                ckw = dict(condition=conds[j][0], unconditional_condition=conds[j][1]) if cfg else {}
                handles[pool.submit(xs[j], blend=mb, **kw, **ckw)] = j
        nets, calls, blends = len(NET_CALLS), len(TBD.CALLS), len(TBD.BLENDS)
        waiting = [q.blend is not None for q in pool._wait]
        done = pool.step()
        if len(NET_CALLS) > nets:
            assert NET_CALLS[nets:] == [80 if cfg else 40]                      # ONE network call per tick, on the whole slab
            R = TBD.CALLS[calls][0]
            assert TBD.CALLS[calls:] == [(R, FILL_B), (R, LAUNCH_B)]            # exactly two multi-request calls, flagged
        else:
            assert TBD.CALLS[calls:] == []
        # stand-alone blends on admitting ticks only, and only for inpainting requests
        admitted = len(waiting) - len(pool._wait)
        if not any(waiting[:admitted]):
            assert len(TBD.BLENDS) == blends
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(reqs)))
    assert not pool._blends and TBD.BLENDS, "the pool keeps no blend of a finished request"
    # the table kernel's rows were there: launches whose header counts a run, with blend rows in them
    assert any(runs >= 1 and nb > 0 for runs, nb, _ in TBD.RUNS)
    NET_CALLS.clear()
    for j, (_, kw, b, mb) in enumerate(reqs):
        cs = [c.expand(b, -1) for c in conds[j]] if cfg else []
        alone = _solver(cfg, dtype, *cs, cxt=mb)
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b)
        if mb is not None:       # (the blend is there: the same request without it ends elsewhere)
            assert not torch.equal(got[j], _solver(cfg, dtype, *cs).sample(xs[j], **kw)), j


def test_steady_state_is_one_copy_per_tick_and_no_blend_launch(doubles):
    dpm = _solver(False, torch.float32)
    g = torch.Generator().manual_seed(1)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), *SHAPE, generator=g) for j in range(10)]
    mbs = [D.MaskBlend(NS, (torch.rand(SHAPE[1:], generator=g) > 0.5).float(), x0=torch.randn_like(x), noise=torch.randn_like(x))
           for x in xs]
    pool = dpm.request_pool(slots=40, inpaint=True)
    hs = [pool.submit(x, steps=8, order=2, blend=mb) for x, mb in zip(xs, mbs)]
    done = dict(pool.step())                       # the admitting tick: table + its own time vector, the blends of x_T
    assert pool.copies == 2
    # one launch per run of consecutive rows (here: per request), a [H,W] mask at its own period
    assert TBD.BLENDS == [(x.numel(), 64) for x in xs]
    for _ in range(4):
        done.update(pool.step())
    assert pool.copies == 6 and TBD.CALLS[-2:] == [(20, FILL_B), (20, LAUNCH_B)]
    assert TBD.RUNS[-1] == (1, 20, 0) and len(TBD.BLENDS) == 10                 # 20 blend rows, ONE run; no further blend launch
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 40 * (L.TABLE_ROW_BYTES + L.TABLE_BLEND_BYTES) + 15) // 16 * 16
    while pool:
        done.update(pool.step())
    for h, x, mb in zip(hs, xs, mbs):
        assert torch.equal(done[h], _solver(False, torch.float32, cxt=mb).sample(x, steps=8, order=2))


def test_a_ragged_mask_period_is_expanded_to_the_sample(doubles):
    """a [W] mask of 6 elements: no multiple of 8 -- the pool's rows carry it expanded to the whole sample"""
    shape = (2, 4, 6)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, *shape, generator=g)
    mb = D.MaskBlend(NS, (torch.rand(6, generator=g) > 0.5).float(), x0=torch.randn(3, *shape, generator=g),
                     noise=torch.randn(3, *shape, generator=g))
    dpm = _solver(False, torch.float32)
    pool = dpm.request_pool(slots=4, inpaint=True)
    h = pool.submit(x, steps=5, order=2, blend=mb)
    done = {}
    while pool:
        done.update(pool.step())
    assert set(pool._bper[:3].tolist()) == {48} and TBD.RUNS[-1][0] == 1
    assert torch.equal(done[h], _solver(False, torch.float32, cxt=mb).sample(x, steps=5, order=2))


def test_an_sde_and_inpainting_pool_runs_sde_blend_and_plain_rows_in_one_tick(monkeypatch):
    """request_pool(slots=S, sde=True, inpaint=True): the tick's calls carry both flags, the table both record sections; SDE
    requests, inpainting requests and plain ones side by side, each the bits of its own call"""
    TBD.install_table_blend_sde_double(monkeypatch, S, D)
    NET_CALLS.clear()
    both = L.TABLE_NOISE | L.TABLE_BLEND
    g = torch.Generator().manual_seed(17)
    dpm = _solver(False, torch.float32)
    pool = dpm.request_pool(slots=12, sde=True, inpaint=True)
    xs = [2.0 * torch.randn(b, *SHAPE, generator=g) for b in (2, 3, 1, 2, 3)]
    mbs = [D.MaskBlend(NS, (torch.rand((b,) + SHAPE, generator=g) > 0.5).float(), x0=torch.randn(b, *SHAPE, generator=g),
                       noise=torch.randn(b, *SHAPE, generator=g)) for b in (3, 2)]
    hs = [pool.submit(xs[0], steps=6, order=2, sde=True, seed=77), pool.submit(xs[1], steps=5, order=3, blend=mbs[0]),
          pool.submit(xs[2], steps=4, order=2), pool.submit(xs[3], steps=7, order=2, blend=mbs[1], denoise_to_zero=True),
          pool.submit(xs[4], steps=5, order=1, sde=True, seed=(1 << 63) + 5)]
    done = {}
    while pool:
        calls = len(TBD.CALLS)
        done.update(pool.step())
        R = TBD.CALLS[calls][0]
        assert TBD.CALLS[calls:] == [(R, L.TABLE_FILL | both), (R, L.TABLE_LAUNCH | both)]
    assert pool._tabb == (L.TABLE_HEADER_BYTES + 12 * (L.TABLE_ROW_BYTES + L.TABLE_NOISE_BYTES + L.TABLE_BLEND_BYTES) + 15) // 16 * 16
    assert TBD.RUNS[0] == (2, 5, 6)                               # an SDE run and a blend run; the lone plain row owns no row
    assert torch.equal(done[hs[0]], dpm.sample_sde(xs[0], steps=6, order=2, seed=77))
    assert torch.equal(done[hs[1]], _solver(False, torch.float32, cxt=mbs[0]).sample(xs[1], steps=5, order=3))
    assert torch.equal(done[hs[2]], dpm.sample(xs[2], steps=4, order=2))
    assert torch.equal(done[hs[3]], _solver(False, torch.float32, cxt=mbs[1]).sample(xs[3], steps=7, order=2, denoise_to_zero=True))
    assert torch.equal(done[hs[4]], dpm.sample_sde(xs[4], steps=5, order=1, seed=(1 << 63) + 5))


# ---- refusals, on a HOST x with no double installed: the device requirement (a RuntimeError) would come first if any device
# work preceded them
def test_every_refusal_comes_before_any_device_work():
    x = torch.randn(2, *SHAPE)
    mask = torch.ones(SHAPE[1:])
    mb = D.MaskBlend(NS, mask, x0=torch.randn(2, *SHAPE), noise=torch.randn(2, *SHAPE))
    dpm = _solver(False, torch.float32)
    with pytest.raises(ValueError, match="inpaint=True belongs to a slab pool"):
        dpm.request_pool(inpaint=True)
    with pytest.raises(NotImplementedError, match="inpaint=True with thresholding=True"):
        dpm.request_pool(slots=8, inpaint=True, thresholding=True)
    # a blend in a pool built without the flag
    with pytest.raises(NotImplementedError, match="inpaint=True"):
        dpm.request_pool(slots=8).submit(x, steps=6, blend=mb)
    with pytest.raises(NotImplementedError, match="inpaint=True"):
        dpm.request_pool(slots=8, sde=True).submit(x, steps=6, blend=mb)
    pool = dpm.request_pool(slots=8, inpaint=True)
    assert isinstance(pool, SlabPool)
    # MaskBlend(x0=..., noise=None) draws per call
    with pytest.raises(NotImplementedError, match="pass noise="):
        pool.submit(x, steps=6, blend=D.MaskBlend(NS, mask, x0=torch.randn(2, *SHAPE)))
    # with sde=True
    with pytest.raises(NotImplementedError, match="blend= with sde=True"):
        dpm.request_pool(slots=8, inpaint=True, sde=True).submit(x, steps=6, order=2, sde=True, seed=1, blend=mb)
    with pytest.raises(NotImplementedError, match="MaskBlend"):
        pool.submit(x, steps=6, blend=lambda x, t, step: x)
    with pytest.raises(TypeError):
        pool.submit_unipc(x, steps=6, blend=mb)
    # without a blend such a pool refuses what every slab pool refuses
    with pytest.raises(NotImplementedError, match="singlestep or adaptive"):
        pool.submit(x, steps=6, method="singlestep", blend=mb)
    with pytest.raises(NotImplementedError, match="correcting_x0_fn / correcting_xt_fn"):
        _solver(False, torch.float32, cxt=mb).request_pool(slots=8, inpaint=True).submit(x, steps=6)
    # ... and a well-formed request on the host then meets the device requirement
    for kw in (dict(blend=mb), dict(blend=D.MaskBlend(NS, mask, intermediates=[torch.randn(2, *SHAPE)] * 8)), dict()):
        with pytest.raises(RuntimeError, match="no CPU fallback|There is no"):
            dpm.request_pool(slots=8, inpaint=True).submit(x, steps=6, **kw)
    assert not pool and pool.step() == {}
