"""A CFG-Zero* slab pool (DPM_Solver.request_pool(slots=S, zero_star=True)) on the MI355X: 8 rows, 12 staggered submits with
steps 4..9 and orders 1..3, one or three samples per request -- so requests wait and rows are reused --, every request with its
own conditions, guidance scale and choice (zero_star=True / False: CFG-Zero* rows and plain rows in one tick), one with
denoise_to_zero, fp32 and fp16, samples of [4,8,8] and SD's [4,64,64].  Every result must equal eager sample() on the request
alone -- a solver whose wrapper has the request's scale and cfg_zero_star (or not) -- bit for bit; a tick is ONE network call on
the whole slab and launches at most one stage_zstar_kernel_table and one plain table kernel.
Run on an MI355X:  pytest -m gpu
"""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
from dpm_solver_amd.slab import SlabPool
from test_gpu_slab_pool import _net
from test_gpu_table_zstar import names_of

gpu = pytest.mark.gpu
DEV = "cuda:0"
NET_CALLS = []
SCALES = (1.5, 3.0, 7.5)


def _counted(x, t, c=None):
    NET_CALLS.append(int(x.shape[0]))
    return _net(x, t, c)


def _solver(dtype, scale=3.0, zstar=False, cond=None, uncond=None):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    fn = D.model_wrapper(_counted, ns, guidance_type="classifier-free", guidance_scale=scale,
                         condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    return D.DPM_Solver(D.cfg_zero_star(fn) if zstar else fn, ns, algorithm_type="dpmsolver++", **kw)


def _requests(n, shape, seed=217):
    """(tick of submission, kwargs, b, guidance scale, choice): steps 4..9, orders 1..3, b in {1, 3}, one with denoise_to_zero
    per ten; scale and choice rotate at different rates"""
    out = []
    for j in range(n):
        kw = dict(steps=4 + j % 6, order=1 + (j // 2) % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 0],
                  denoise_to_zero=(j % 10 == 0))
        out.append((j // 3, kw, 1 + 2 * (j % 3 == 1), SCALES[j % 3], (True, True, False, True)[(j + j // 3) % 4]))
    g = torch.Generator().manual_seed(seed)
    xs = [2.0 * torch.randn((b,) + shape, generator=g) for _, _, b, _, _ in out]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b, _, _) in enumerate(out)]
    return out, xs, conds


@gpu
@pytest.mark.parametrize("dtype,shape", [(torch.float32, (4, 8, 8)), (torch.float16, (4, 8, 8)),
                                         (torch.float32, (4, 64, 64)), (torch.float16, (4, 64, 64))],
                         ids=["f32-256", "f16-256", "f32-16384", "f16-16384"])
def test_staggered_zstar_slab_pool_equals_every_request_alone(dtype, shape):
    reqs, xs, conds = _requests(12, shape)
    assert {r[4] for r in reqs} == {True, False} and {r[3] for r in reqs} == set(SCALES)
    assert any(r[1]["denoise_to_zero"] and r[4] for r in reqs)
    xs = [x.to(DEV).to(dtype) for x in xs]
    conds = [(c.to(DEV), u.to(DEV)) for c, u in conds]
    dpm = _solver(dtype, 3.0, False)
    pool = dpm.request_pool(slots=8, zero_star=True)
    assert isinstance(pool, SlabPool)
    handles, got, tick, waited, launches = {}, {}, 0, False, []
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kw, b, s, on) in enumerate(reqs):
            if t == tick:
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], guidance_scale=s,
                                    zero_star=on, **kw)] = j
        nets = len(NET_CALLS)
        if tick == 4:                                              # one mixed tick under the profiler, by kernel name
            # (names_of runs its function twice: the first tick outside the profile)
            launches = names_of(lambda: [got.__setitem__(handles[h], out) for h, out in pool.step().items()])
            assert NET_CALLS[nets:] == [16, 16], "a tick is ONE network call on the whole slab"
        else:
            for h, out in pool.step().items():
                got[handles[h]] = out
            assert NET_CALLS[nets:] == [16], "a tick is ONE network call on the whole slab"
        waited = waited or bool(pool._wait)
        tick += 1
    assert sorted(got) == list(range(len(reqs))) and waited
    # at most one CFG-Zero* table kernel and one plain table kernel per tick; the rest (plain rows of a group too small for
    # rows) as a RequestPool launches them
    assert sum("stage_zstar_kernel_table" in n for n in launches) == 1, launches
    assert sum("stage_kernel_table" in n for n in launches) <= 1, launches
    assert not any("stage_zstar_kernel<" in n for n in launches), launches
    for j, (_, kw, b, s, on) in enumerate(reqs):
        alone = _solver(dtype, s, on, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, s, on)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_steady_tick_of_zstar_rows_is_one_network_call_one_launch_and_one_copy(dtype):
    dpm = _solver(dtype, 7.5, True)
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 64, 64, generator=g, device=DEV).to(dtype) for j in range(10)]      # 20 rows
    pool = dpm.request_pool(slots=24, zero_star=True)
    hs = [pool.submit(x, steps=6 + j % 3, order=1 + j % 3, **(dict(guidance_scale=SCALES[j % 3]) if j % 2 else {}))
          for j, x in enumerate(xs)]
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    names = []
    for _ in range(2):
        assert len(pool) == 10
        nets = len(NET_CALLS)
        names.append(names_of(lambda: done.update(pool.step())))
        assert NET_CALLS[nets:] == [48, 48]
    assert all(len(n) == 1 and "stage_zstar_kernel_table" in n[0] for n in names), names
    assert pool.copies == 6                                 # one per tick, and the admitting tick's time vector
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        alone = _solver(dtype, SCALES[j % 3], True) if j % 2 else dpm
        assert torch.equal(done[h], alone.sample(x, steps=6 + j % 3, order=1 + j % 3)), j
