"""An inpainting slab pool (DPM_Solver.request_pool(slots=S, inpaint=True)) on the MI355X: 40 rows, staggered submits with steps
4..9 and orders 1..3, one or three samples per request, denoise_to_zero on some, unconditional and classifier-free with
per-request conditions, fp32 and fp16, samples of [4,16,16] and [4,64,64]; both MaskBlend modes, masks [H,W], [1,C,H,W] and
full size, a time_fn on some, plain requests mixed in.  Every result must equal the request's own sample() -- of a solver built
with correcting_xt_fn=mb -- bit for bit; a steady tick is ONE network call and ONE stage_kernel_table_blend launch.
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
_BETAS = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
NS = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - _BETAS).astype(np.float32)))


def _counted(x, t, c=None):
    NET_CALLS.append(int(x.shape[0]))
    return _net(x, t, c)


def _solver(cfg, dtype, cond=None, uncond=None, cxt=None):
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    if cfg:
        fn = D.model_wrapper(_counted, NS, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                             unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    else:
        fn = D.model_wrapper(_counted, NS)
    return D.DPM_Solver(fn, NS, algorithm_type="dpmsolver++", correcting_xt_fn=cxt, **kw)


def _time_fn(t):
    return 0.5 * t + 0.25


def _requests(n, shape, dtype, seed=211):
    """the staggered pool of tests/test_slab_inpaint_host.py: (tick of submission, kwargs, b, MaskBlend or None)"""
    g = torch.Generator().manual_seed(seed)
    dev = lambda t: t.to(DEV).to(dtype)
    out = []
    for j in range(n):
        steps, b = 4 + j % 6, 1 + 2 * (j % 3 == 1)
        kw = dict(steps=steps, order=1 + (j // 2) % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 0],
                  denoise_to_zero=(j % 7 == 3))
        mshape = (shape[1:], (1,) + shape, (b,) + shape)[j % 3]
        mask = dev((torch.rand(mshape, generator=g) > 0.5).float())
        if j % 5 == 0:
            mb = None
        elif j % 5 in (1, 3):
            mb = D.MaskBlend(NS, mask, x0=dev(torch.randn((b,) + shape, generator=g)),
                             noise=dev(torch.randn((b,) + shape, generator=g)), time_fn=_time_fn if j % 4 == 1 else None)
        else:
            mb = D.MaskBlend(NS, mask, intermediates=[dev(torch.randn((b,) + shape, generator=g)) for _ in range(steps + 2)])
        out.append((j // 4, kw, b, mb))
    xs = [dev(2.0 * torch.randn((b,) + shape, generator=g)) for _, _, b, _ in out]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g).to(DEV), (torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0).to(DEV))
             for j, (_, _, b, _) in enumerate(out)]
    return out, xs, conds


@gpu
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype,shape,n", [(torch.float32, (4, 16, 16), 30), (torch.float16, (4, 16, 16), 30),
                                           (torch.float32, (4, 64, 64), 12), (torch.float16, (4, 64, 64), 12)],
                         ids=["f32-1024", "f16-1024", "f32-16384", "f16-16384"])
def test_staggered_inpainting_slab_pool_equals_every_request_alone(dtype, shape, n, cfg):
    reqs, xs, conds = _requests(n, shape, dtype)
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=40, inpaint=True)
    assert isinstance(pool, SlabPool)
    handles, got, tick = {}, {}, 0
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kw, b, mb) in enumerate(reqs):
            if t == tick:
                ckw = dict(condition=conds[j][0], unconditional_condition=conds[j][1]) if cfg else {}
                handles[pool.submit(xs[j], blend=mb, **kw, **ckw)] = j
        nets = len(NET_CALLS)
        for h, out in pool.step().items():
            got[handles[h]] = out
        assert NET_CALLS[nets:] == [80 if cfg else 40], "a tick is ONE network call on the whole slab"
        tick += 1
    assert sorted(got) == list(range(len(reqs))) and not pool._blends
    for j, (_, kw, b, mb) in enumerate(reqs):
        cs = [c.expand(b, -1) for c in conds[j]] if cfg else []
        want = _solver(cfg, dtype, *cs, cxt=mb).sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b)
        if mb is not None:
            assert not torch.equal(got[j], _solver(cfg, dtype, *cs).sample(xs[j], **kw)), j


@gpu
@pytest.mark.parametrize("plain", [False, True], ids=["blend", "blend+plain"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_steady_tick_is_one_network_call_and_one_table_blend_launch(dtype, plain):
    dpm = _solver(False, dtype)
    g = torch.Generator(device=DEV).manual_seed(5)
    shape = (4, 64, 64)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), *shape, generator=g, device=DEV).to(dtype) for j in range(10)]      # 20 rows
    mbs = [D.MaskBlend(NS, (torch.rand(shape[1:] if j % 2 else shape, generator=g, device=DEV) > 0.5).to(dtype),
                       x0=torch.randn_like(x), noise=torch.randn_like(x)) for j, x in enumerate(xs)]
    pool = dpm.request_pool(slots=40, inpaint=True)
    hs = [pool.submit(x, steps=6 + j % 3, order=1 + j % 3, blend=mb) for j, (x, mb) in enumerate(zip(xs, mbs))]
    extra = [2.0 * torch.randn(1, *shape, generator=g, device=DEV).to(dtype) for _ in range(18 if plain else 0)]
    hp = [pool.submit(x, steps=7, order=2) for x in extra]     # 18 plain rows: a run of their own in the plain family's kernel
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    names = []
    for _ in range(2):
        assert len(pool) == 10 + len(extra)
        nets = len(NET_CALLS)
        # (_names runs its function twice: once outside the profile)
        names.append(_names(lambda: done.update(pool.step())))
        assert NET_CALLS[nets:] == [40, 40]
    for n in names:
        assert sum("stage_kernel_table_blend" in k for k in n) == 1 and len(n) == (2 if plain else 1), names
        assert not plain or sum("stage_kernel_table<" in k for k in n) == 1, names
    assert pool.copies == 6                                 # one per tick, and the admitting tick's time vector
    while pool:
        done.update(pool.step())
    for j, (h, x, mb) in enumerate(zip(hs, xs, mbs)):
        assert torch.equal(done[h], _solver(False, dtype, cxt=mb).sample(x, steps=6 + j % 3, order=1 + j % 3)), j
    for h, x in zip(hp, extra):
        assert torch.equal(done[h], dpm.sample(x, steps=7, order=2))
