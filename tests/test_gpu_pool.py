"""GPU tests of DPM_Solver.request_pool (continuous batching): 32 requests of [256,4,64,64], admitted at staggered ticks with
their own step counts, orders and methods, each bit-identical to sample(); staggered 2M ticks of fusable requests are
one fused kernel launch per tick.  Run on an MI355X:  pytest -m gpu
"""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (256, 4, 64, 64)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    yield
    torch.cuda.synchronize()


def sd_schedule():
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))


def solver(cfg=False, algorithm_type="dpmsolver++"):
    ns = sd_schedule()
    if cfg:
        c = torch.ones(SHAPE[0], device=DEV)
        fn = D.model_wrapper(lambda x, t, cond: x * 0.9 + 0.05 * cond.reshape(-1, 1, 1, 1)[:x.shape[0]], ns,
                             guidance_type="classifier-free", guidance_scale=4.0, condition=c, unconditional_condition=c * 0)
    else:
        fn = D.model_wrapper(lambda x, t: x * 0.9 + 0.01 * t.reshape(-1, 1, 1, 1), ns)
    return D.DPM_Solver(fn, ns, algorithm_type=algorithm_type)


KW = [dict(steps=20, order=2), dict(steps=15, order=3), dict(steps=8, order=2), dict(steps=6, order=1),
      dict(steps=12, order=3, method="singlestep"), dict(steps=9, order=2, denoise_to_zero=True),
      dict(steps=10, order=2, skip_type="logSNR"), dict(steps=7, order=3, lower_order_final=False)]


def run_pool(dpm, xs, kws, ticks):
    pool = dpm.request_pool()
    handles, got, tick = {}, {}, 0
    while tick <= max(ticks) or pool:
        for j, t in enumerate(ticks):
            if t == tick:
                handles[pool.submit(xs[j], **kws[j])] = j
        for h, out in pool.step().items():
            got[handles[h]] = out
        tick += 1
    return got


@pytest.mark.parametrize("dtype,cfg", [(torch.float16, False), (torch.float32, False), (torch.float16, True)])
def test_pool_32_requests_equal_sample(dtype, cfg):
    dpm = solver(cfg=cfg)
    g = torch.Generator(device=DEV).manual_seed(11)
    R = 32
    kws = [KW[j % len(KW)] for j in range(R)]
    ticks = [(j * 5) % 13 for j in range(R)]
    xs = [torch.randn(SHAPE, generator=g, device=DEV).to(dtype) for _ in range(R)]
    got = run_pool(dpm, xs, kws, ticks)
    assert sorted(got) == list(range(R))
    for j in range(R):
        want = dpm.sample(xs[j], **kws[j])
        assert got[j].dtype == want.dtype and torch.equal(got[j], want), (j, kws[j])


def test_pool_staggered_2m_ticks_are_one_launch():
    """16 fusable requests (dpmsolver++ 2M, fp16) at 16 different positions: every tick is one stage_kernel_het launch"""
    from torch.profiler import ProfilerActivity, profile
    dpm = solver()
    g = torch.Generator(device=DEV).manual_seed(2)
    R, steps = 16, 20
    pool = dpm.request_pool()
    for j in range(R):                    # one admission per tick: positions 0 .. 15 after the ramp
        pool.submit(torch.randn(SHAPE, generator=g, device=DEV).half(), steps=steps, order=2)
        pool.step()
    torch.cuda.synchronize()
    ticks = 3                             # the oldest request is at stage 16 of 20: none finishes during these ticks
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(ticks):
            pool.step()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if "stage_kernel" in e.key for _ in range(e.count)]
    assert len(names) == ticks and all("stage_kernel_het" in n for n in names), names
    assert len(pool) == R
