"""The slab pool (DPM_Solver.request_pool(slots=S)) on the MI355X: the staggered scenario of tests/test_slab_pool_host.py on the
device -- 40 small requests in 32 rows, 2M-style multistep and UniPC, unconditional and classifier-free with per-request
conditions, fp32 and fp16 -- with an elementwise network of the row's state, time and condition.  Every result must equal the
request's own sample() / sample_unipc() bit for bit, and a tick with more than 16 rows of one group is ONE stage_kernel_table
launch.
Run on an MI355X:  pytest -m gpu
"""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
from dpm_solver_amd.slab import SlabPool
from test_gpu_unipc_pool import _stage_kernels
from test_slab_pool_host import _requests

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _net(x, t, c=None):
    xf = x.float()
    out = 0.5 * xf + 0.1 * torch.sin(xf) + 0.0001 * t.float().reshape(-1, 1, 1, 1)
    if c is not None:
        out = out * (0.8 + 0.2 * c.float().repeat_interleave(x.shape[0] // c.shape[0], dim=0).reshape(-1, 1, 1, 1))
    return out.to(x.dtype)


def _solver(cfg, dtype, cond=None, uncond=None):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_net, ns, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_net, ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", **kw)


@gpu
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_slab_pool_equals_every_request_alone(dtype, cfg):
    reqs, xs, conds = _requests(40)
    xs = [x.to(DEV).to(dtype) for x in xs]
    conds = [(c.to(DEV), u.to(DEV)) for c, u in conds]
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=32)
    assert isinstance(pool, SlabPool)
    handles, got, tick = {}, {}, 0
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kind, kw, b) in enumerate(reqs):
            if t == tick:
                ckw = dict(condition=conds[j][0], unconditional_condition=conds[j][1]) if cfg else {}
                handles[(pool.submit_unipc if kind == "unipc" else pool.submit)(xs[j], **kw, **ckw)] = j
        for h, out in pool.step().items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(reqs)))
    for j, (_, kind, kw, b) in enumerate(reqs):
        alone = _solver(cfg, dtype, *[c.expand(b, -1) for c in conds[j]]) if cfg else dpm
        want = (alone.sample_unipc if kind == "unipc" else alone.sample)(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, (j, kind, kw)
        assert torch.equal(got[j], want), (j, kind, kw, b)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_tick_of_more_than_16_rows_is_one_table_launch(dtype):
    dpm = _solver(False, dtype)
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [torch.randn(1 + j % 2, 4, 16, 16, generator=g, device=DEV).to(dtype) for j in range(14)]      # 21 rows
    pool = dpm.request_pool(slots=32)
    hs = [pool.submit(x, steps=6 + j % 3, order=2) for j, x in enumerate(xs)]
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    names = []
    for _ in range(4):
        assert len(pool) == 14
        names.append(_stage_kernels(lambda: done.update(pool.step())))
    assert all(len(n) == 1 and "stage_kernel_table<" in n[0] for n in names), names
    assert pool.copies == 6                                 # one per tick, and the admitting tick's time vector
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        assert torch.equal(done[h], dpm.sample(x, steps=6 + j % 3, order=2)), j
