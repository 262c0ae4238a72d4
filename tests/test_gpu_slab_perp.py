"""A Perp-Neg slab pool (DPM_Solver.request_pool(slots=S, perp_neg=True)) on the MI355X: the staggered pool of
tests/test_slab_perp_host.py on the device -- 8 rows, 12 submits with steps 4..9 and orders 1..3, one or three samples per request,
so requests wait and rows are reused; every request with its own three conditions, guidance scale and negative scale; one with
denoise_to_zero; fp32 and fp16, samples of [4,8,8] and SD's [4,64,64], and [4,72,64] in fp16 (18432 elements: the kernel's
re-read path).  Every result must equal eager sample() on the request alone -- a solver whose wrapper is
cfg_perp_neg(model_wrapper(..., guidance_scale=s, condition=c, unconditional_condition=u), n, w) -- bit for bit; a tick is ONE
network call on the whole [3S] slab and ONE stage_perp_kernel_table launch per group, never a lone stage_perp_kernel and never a
`cat`.
Run on an MI355X:  pytest -m gpu
"""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
from dpm_solver_amd.slab import SlabPool
from test_gpu_table_zstar import names_of
from test_slab_perp_host import OWN, REQS, SLOTS

gpu = pytest.mark.gpu
DEV = "cuda:0"
NET_CALLS = []


def _net(x, t, c):
    """elementwise in the row -- its state, its time, its condition --, in exactly rounded operations, not linear in the condition"""
    NET_CALLS.append(int(x.shape[0]))
    xf = x.float()
    xc = torch.clamp(xf, -2.0, 2.0)
    cc = c.float().repeat_interleave(x.shape[0] // c.shape[0], dim=0).reshape(-1, 1, 1, 1)
    out = xf * (0.5 + 0.1 * cc) + 0.1 * xc * xc * cc * cc + 0.05 * cc + 0.0001 * t.float().reshape(-1, 1, 1, 1)
    return out.to(x.dtype)


def _solver(dtype, s=3.0, w=1.5, cond=None, uncond=None, neg=None):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=s,
                         condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    fn = D.cfg_perp_neg(fn, torch.full((1, 1), 0.5, device=DEV) if neg is None else neg, w)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", **kw)


def _kernels(fn):
    """names of every GPU kernel fn() launches (torch's profiler), one entry per launch"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() for _ in range(e.count)]


@gpu
@pytest.mark.parametrize("dtype,shape", [(torch.float32, (4, 8, 8)), (torch.float16, (4, 8, 8)),
                                         (torch.float32, (4, 64, 64)), (torch.float16, (4, 64, 64)),
                                         (torch.float16, (4, 72, 64))],
                         ids=["f32-256", "f16-256", "f32-16384", "f16-16384", "f16-18432"])
def test_staggered_perp_slab_pool_equals_every_request_alone(dtype, shape):
    g = torch.Generator().manual_seed(221)
    xs = [(2.0 * torch.randn((b,) + shape, generator=g)).to(DEV).to(dtype) for _, _, b in REQS]
    conds = [tuple(c.to(DEV) for c in (torch.rand(b if j % 2 else 1, 1, generator=g),
                                       torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0,
                                       torch.rand(b if j % 4 == 2 else 1, 1, generator=g) + 0.5))
             for j, (_, _, b) in enumerate(REQS)]
    dpm = _solver(dtype)
    pool = dpm.request_pool(slots=SLOTS, perp_neg=True)
    assert isinstance(pool, SlabPool)
    handles, got, tick, waited, launches = {}, {}, 0, False, []
    while tick <= max(r[0] for r in REQS) or pool:
        for j, (t, kw, b) in enumerate(REQS):
            if t == tick:
                s, w = OWN[j]
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1],
                                    negative_condition=conds[j][2], guidance_scale=s, neg_scale=w, **kw)] = j
        nets = len(NET_CALLS)
        if tick == 3:                                              # one mixed tick under the profiler, by kernel name
            # (names_of runs its function twice: the first tick outside the profile)
            launches = names_of(lambda: [got.__setitem__(handles[h], out) for h, out in pool.step().items()])
            assert NET_CALLS[nets:] == [3 * SLOTS] * 2, "a tick is ONE network call on the whole slab"
        else:
            for h, out in pool.step().items():
                got[handles[h]] = out
            assert NET_CALLS[nets:] == [3 * SLOTS], "a tick is ONE network call on the whole slab"
        waited = waited or bool(pool._wait)
        tick += 1
    assert sorted(got) == list(range(len(REQS))) and waited
    assert sum("stage_perp_kernel_table" in n for n in launches) == 1, launches
    assert not any("stage_perp_kernel<" in n or "stage_pair_kernel" in n for n in launches), launches
    for j, (_, kw, b) in enumerate(REQS):
        s, w = OWN[j]
        alone = _solver(dtype, s, w, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, OWN[j])


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_steady_tick_of_perp_rows_is_one_network_call_one_launch_one_copy_and_no_cat(dtype):
    dpm = _solver(dtype, 7.5, 1.0)
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 64, 64, generator=g, device=DEV).to(dtype) for j in range(10)]      # 20 rows
    pool = dpm.request_pool(slots=24, perp_neg=True)
    hs = [pool.submit(x, steps=6 + j % 3, order=2, **(dict(guidance_scale=OWN[j][0], neg_scale=OWN[j][1]) if j % 2 else {}))
          for j, x in enumerate(xs)]
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    done.update(pool.step())
    for _ in range(2):
        assert len(pool) == 10
        nets = len(NET_CALLS)
        names = _kernels(lambda: done.update(pool.step()))
        assert NET_CALLS[nets:] == [72]
        stage = [n for n in names if "stage_" in n and "kernel" in n]
        assert len(stage) == 1 and "stage_perp_kernel_table" in stage[0], names
        assert not any("CatArray" in n for n in names), names          # no torch.cat builds the network's next input
    assert pool.copies == 5                                 # one per tick, and the admitting tick's time vector
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        alone = _solver(dtype, *OWN[j]) if j % 2 else dpm
        assert torch.equal(done[h], alone.sample(x, steps=6 + j % 3, order=2)), j
