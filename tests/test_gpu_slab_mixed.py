"""A slab pool that holds EVERY kind of request at once (DPM_Solver.request_pool(slots=12, sde=True, inpaint=True)) on the MI355X:
the churn scenario of tests/mixed_pool_cases.py -- 36 plain, UniPC, SDE and inpainting requests through 12 rows, rows changing
kind as they are freed and handed on, the lowest active row of every kind in turn -- for fp32 and fp16, unconditional and
classifier-free with per-request conditions, samples of [4,16,16]; and its first 12 requests at [4,64,64] in fp16.  Every result
must equal the request run alone on the GPU bit for bit (sample / sample_unipc / sample_sde(seed=) / sample of a solver built
with correcting_xt_fn=mb); every tick is ONE network call on the whole slab; on two ticks with all four kinds active the
launches are counted by kernel name against the grouping rule restated in mixed_pool_cases.expected_launches; a tick that admits
nobody issues one host-to-device copy.  The same in small for a thresholding pool built with sde=True: one
stage_thresh_kernel_table launch per tick.
Run on an MI355X:  pytest -m gpu
"""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import mixed_pool_cases as M
from dpm_solver_amd.slab import SlabPool
from test_gpu_slab_pool import _net

gpu = pytest.mark.gpu
DEV = "cuda:0"
NET_CALLS = []
_BETAS = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
NS = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - _BETAS).astype(np.float32)))


def _counted(x, t, c=None):
    NET_CALLS.append(int(x.shape[0]))
    return _net(x, t, c)


def _solver(cfg, dtype, cond=None, uncond=None, cxt=None, thresholding=False):
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_counted, NS, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_counted, NS)
    return D.DPM_Solver(fn, NS, algorithm_type="dpmsolver++", correcting_xt_fn=cxt,
                        correcting_x0_fn="dynamic_thresholding" if thresholding else None, **kw)


def _tick_kernels(fn):
    """names of the stage kernels ONE call of fn() launches, one entry per launch: _stage_kernels of
    tests/test_gpu_unipc_pool.py with the thresholding family listed too (a tick cannot be run twice)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if "stage_kernel" in e.key or "stage_thresh_kernel" in e.key for _ in range(e.count)]


def _count(names, *parts):
    return sum(any(p in n for p in parts) for n in names)


@gpu
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype,shape,n", [(torch.float32, M.SHAPE, 36), (torch.float16, M.SHAPE, 36), (torch.float16, (4, 64, 64), 12)],
                         ids=["f32-1024", "f16-1024", "f16-16384"])
def test_churning_pool_of_every_kind_equals_every_request_alone(dtype, shape, n, cfg):
    sps = M.specs(M.ORDER[:n])
    sim, admitted = M.simulate(sps)
    counted = M.counting_ticks(sps, sim, admitted)
    assert len(counted) == 2 or n < len(M.ORDER)
    xs, conds, mbs = M.tensors(sps, dtype, DEV, NS, D.MaskBlend, shape=shape)
    pool = _solver(cfg, dtype).request_pool(slots=M.SLOTS, sde=True, inpaint=True)
    assert isinstance(pool, SlabPool)
    names, nets = {}, [0]

    def around_step(tick, step):
        if tick in counted:
            names[tick] = _tick_kernels(step)
        else:
            step()

    def each_tick(tick, occ, info):
        assert NET_CALLS[nets[0]:] == [2 * M.SLOTS if cfg else M.SLOTS], "a tick is ONE network call on the whole slab"
        nets[0] = len(NET_CALLS)
        assert info["copies"] == 1 or (info["admitted"] and info["copies"] == 2), (tick, info)     # a steady tick: one copy
        if tick in counted:
            k, e = names[tick], info["expect"]
            assert M.kinds_active(sps, occ) == set(M.KINDS) and e["noise"] == e["blend"] == 1, (tick, e)
            assert _count(k, "stage_kernel_table_noise") == 1 and _count(k, "stage_kernel_table_blend") == 1, (tick, k)
            # the plain / UniPC rows as the walk groups them: a table launch from 17 members on, a kernarg launch from 2
            assert _count(k, "stage_kernel_table_unipc") == e["table_unipc"] and _count(k, "stage_kernel_table<") == e["table"], (tick, e, k)
            assert _count(k, "stage_kernel_het_unipc") == e["het_unipc"] and _count(k, "stage_kernel_het<") == e["het"], (tick, e, k)
            assert len(k) == sum(e.values()), (tick, e, k)
    nets[0] = len(NET_CALLS)
    got, ticks = M.run(pool, sps, xs, conds, mbs, cfg, each_tick, around_step)
    assert ticks == sim, "mixed_pool_cases.simulate is not the pool's admission rule"
    assert sorted(got) == list(range(len(sps))) and not pool._blends and not pool._ropts
    assert sorted(names) == sorted(counted)
    for sp in sps:
        j = sp["j"]
        want = M.alone(lambda c, u, cxt: _solver(cfg, dtype, c, u, cxt), sp, xs[j], conds[j], mbs[j], cfg)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, sp
        assert torch.equal(got[j], want), sp


@gpu
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_thresholding_pool_built_with_sde_is_one_thresholding_table_launch_per_tick(dtype, cfg):
    sps = M.thresh_specs()
    xs, conds, mbs = M.tensors(sps, dtype, DEV, NS, D.MaskBlend, shape=M.THR_SHAPE)
    dpm = _solver(cfg, dtype, thresholding=True)
    pool = dpm.request_pool(slots=M.THR_SLOTS, thresholding=True, sde=True)
    assert isinstance(pool, SlabPool)
    with pytest.raises(NotImplementedError):                      # its SDE submit stays refused
        pool.submit(xs[0], steps=6, sde=True, seed=1)
    names, nets = {}, [len(NET_CALLS)]

    def around_step(tick, step):
        names[tick] = _tick_kernels(step)

    def each_tick(tick, occ, info):
        assert NET_CALLS[nets[0]:] == [2 * M.THR_SLOTS if cfg else M.THR_SLOTS], "a tick is ONE network call on the whole slab"
        nets[0] = len(NET_CALLS)
        assert len(names[tick]) == 1 and "stage_thresh_kernel_table" in names[tick][0], (tick, names[tick])
        assert info["copies"] == 1 or (info["admitted"] and info["copies"] == 2), (tick, info)
    got, ticks = M.run(pool, sps, xs, conds, mbs, cfg, each_tick, around_step)
    assert ticks == M.simulate(sps, M.THR_SLOTS)[0] and sorted(got) == list(range(len(sps)))
    for sp in sps:
        j = sp["j"]
        want = M.alone(lambda c, u, cxt: _solver(cfg, dtype, c, u, thresholding=True), sp, xs[j], conds[j], None, cfg)
        assert got[j].dtype == want.dtype == dtype and torch.equal(got[j], want), sp
