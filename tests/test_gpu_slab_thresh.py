"""A thresholding slab pool (DPM_Solver.request_pool(slots=S, thresholding=True)) on the MI355X: 40 rows, staggered submits
with steps 4..9 and orders 1..3, one or three samples per request, unconditional and classifier-free with per-request
conditions, fp32 and fp16, a sample of [3,16,16] and the largest a row holds, [3,64,64].  Every result must equal the request's
own sample() bit for bit; a tick is ONE network call and ONE stage_thresh_kernel_table launch.
Run on an MI355X:  pytest -m gpu
"""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
from dpm_solver_amd.slab import SlabPool
from test_gpu_slab_pool import _net
from test_gpu_table_thresh import _names

gpu = pytest.mark.gpu
DEV = "cuda:0"
NET_CALLS = []


def _counted(x, t, c=None):
    NET_CALLS.append(int(x.shape[0]))
    return _net(x, t, c)


def _solver(cfg, dtype, cond=None, uncond=None):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_counted, ns, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_counted, ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding", **kw)


def _requests(n, shape, seed=210):
    """(tick of submission, kwargs, b): steps 4..9, orders 1..3, b in {1, 3}"""
    out = []
    for j in range(n):
        kw = dict(steps=4 + j % 6, order=1 + (j // 2) % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 0],
                  denoise_to_zero=(j % 10 == 0))
        out.append((j // 4, kw, 1 + 2 * (j % 3 == 1)))
    g = torch.Generator().manual_seed(seed)
    xs = [2.0 * torch.randn((b,) + shape, generator=g) for _, _, b in out]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b) in enumerate(out)]
    return out, xs, conds


@gpu
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype,shape,n", [(torch.float32, (3, 16, 16), 30), (torch.float16, (3, 16, 16), 30),
                                           (torch.float16, (3, 64, 64), 12)], ids=["f32-768", "f16-768", "f16-12288"])
def test_staggered_thresholding_slab_pool_equals_every_request_alone(dtype, shape, n, cfg):
    reqs, xs, conds = _requests(n, shape)
    xs = [x.to(DEV).to(dtype) for x in xs]
    conds = [(c.to(DEV), u.to(DEV)) for c, u in conds]
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=40, thresholding=True)
    assert isinstance(pool, SlabPool)
    handles, got, tick = {}, {}, 0
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kw, b) in enumerate(reqs):
            if t == tick:
                ckw = dict(condition=conds[j][0], unconditional_condition=conds[j][1]) if cfg else {}
                handles[pool.submit(xs[j], **kw, **ckw)] = j
        nets = len(NET_CALLS)
        for h, out in pool.step().items():
            got[handles[h]] = out
        assert NET_CALLS[nets:] == [80 if cfg else 40], "a tick is ONE network call on the whole slab"
        tick += 1
    assert sorted(got) == list(range(len(reqs)))
    for j, (_, kw, b) in enumerate(reqs):
        alone = _solver(cfg, dtype, *[c.expand(b, -1) for c in conds[j]]) if cfg else dpm
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_tick_is_one_network_call_and_one_thresholding_table_launch(dtype):
    dpm = _solver(False, dtype)
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 3, 64, 64, generator=g, device=DEV).to(dtype) for j in range(10)]      # 20 rows
    pool = dpm.request_pool(slots=40, thresholding=True)
    hs = [pool.submit(x, steps=6 + j % 3, order=1 + j % 3) for j, x in enumerate(xs)]
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    names = []
    for _ in range(2):
        assert len(pool) == 10
        nets = len(NET_CALLS)
        # (_names runs its function twice: once outside the profile)
        names.append(_names(lambda: done.update(pool.step())))
        assert NET_CALLS[nets:] == [40, 40]
    assert all(len(n) == 1 and "stage_thresh_kernel_table" in n[0] for n in names), names
    assert pool.copies == 6                                 # one per tick, and the admitting tick's time vector
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        assert torch.equal(done[h], dpm.sample(x, steps=6 + j % 3, order=1 + j % 3)), j
