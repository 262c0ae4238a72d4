"""An adaptive-projected-guidance slab pool (DPM_Solver.request_pool(slots=S, apg=True)) on the MI355X: 24 rows, staggered
submits with steps 4..9 and orders 1..3, one or three samples per request, more rows' worth of requests than the pool has rows
(so rows are reused, also by a request with a momentum after another with one), every request with its own conditions,
guidance scale and (eta, norm threshold, momentum) -- with and without a momentum, (1, 0, 0) among them: plain rows --, fp32
and fp16, samples of [4,8,8] and SD's [4,64,64].  Every result must equal sample() on the request alone -- a solver whose
wrapper has the request's scale and cfg_apg(fn, *its parameters) -- bit for bit; a tick is ONE network call on the whole slab,
and a steady tick of APG rows ONE stage_apg_kernel_table launch and ONE copy.
Run on an MI355X:  pytest -m gpu
"""
import numpy as np
import pytest
import torch

import dpm_solver_amd as D
from dpm_solver_amd.slab import SlabPool
from test_gpu_slab_pool import _net
from test_gpu_table_apg import names_of

gpu = pytest.mark.gpu
DEV = "cuda:0"
NET_CALLS = []
SCALES = (1.5, 3.0, 7.5)
PLAIN = (1.0, 0.0, 0.0)
PARAMS = ((0.0, 15.0, -0.5), PLAIN, (0.5, 0.0, 0.0), (0.25, 2.5, 0.25), (1.0, 1e-3, -0.75))


def _counted(x, t, c=None):
    NET_CALLS.append(int(x.shape[0]))
    return _net(x, t, c)


def _solver(dtype, scale=3.0, apg=None, cond=None, uncond=None):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    kw = dict(state_dtype=dtype) if dtype is not torch.float32 else {}
    fn = D.model_wrapper(_counted, ns, guidance_type="classifier-free", guidance_scale=scale,
                         condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    return D.DPM_Solver(fn if apg is None else D.cfg_apg(fn, *apg), ns, algorithm_type="dpmsolver++", **kw)


def _requests(n, shape, seed=215):
    """(tick of submission, kwargs, b, guidance scale, parameters): steps 4..9, orders 1..3, b in {1, 3}, one with
    denoise_to_zero per five; scale and parameters rotate at different rates"""
    out = []
    for j in range(n):
        kw = dict(steps=4 + j % 6, order=1 + (j // 2) % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 0],
                  denoise_to_zero=(j % 5 == 0))
        out.append((j // 3, kw, 1 + 2 * (j % 3 == 1), SCALES[j % 3], PARAMS[(j + j // 5) % 5]))
    g = torch.Generator().manual_seed(seed)
    xs = [2.0 * torch.randn((b,) + shape, generator=g) for _, _, b, _, _ in out]
    conds = [(torch.rand(b if j % 2 else 1, 1, generator=g), torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0)
             for j, (_, _, b, _, _) in enumerate(out)]
    return out, xs, conds


@gpu
@pytest.mark.parametrize("wrapper_apg", [None, (0.5, 10.0, -0.25)], ids=["wplain", "wapg"])
@pytest.mark.parametrize("dtype,shape,n", [(torch.float32, (4, 8, 8), 24), (torch.float16, (4, 8, 8), 24),
                                           (torch.float32, (4, 64, 64), 24), (torch.float16, (4, 64, 64), 24)],
                         ids=["f32-256", "f16-256", "f32-16384", "f16-16384"])
def test_staggered_apg_slab_pool_equals_every_request_alone(dtype, shape, n, wrapper_apg):
    reqs, xs, conds = _requests(n, shape)
    assert {r[4] for r in reqs} == set(PARAMS) and {r[3] for r in reqs} == set(SCALES)
    assert any(r[1]["denoise_to_zero"] and r[4][2] != 0 for r in reqs)        # a DENOISE stage that updates an average
    assert sum(r[2] for r in reqs) > 24                                       # more rows' worth of requests than rows
    xs = [x.to(DEV).to(dtype) for x in xs]
    conds = [(c.to(DEV), u.to(DEV)) for c, u in conds]
    dpm = _solver(dtype, 3.0, wrapper_apg)
    pool = dpm.request_pool(slots=24, apg=True)
    assert isinstance(pool, SlabPool)
    handles, got, tick, rows_of, used = {}, {}, 0, {}, {}
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kw, b, s, par) in enumerate(reqs):
            if t == tick:
                okw = dict(guidance_scale=s, apg=par)
                if j % 7 == 3:
                    del okw["apg"]                                            # the request's scale, the wrapper's parameters
                    par = wrapper_apg or PLAIN
                if j % 7 == 5:
                    del okw["guidance_scale"]                                 # the wrapper's scale, the request's parameters
                    s = 3.0
                used[j] = (s, par)
                handles[pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], **okw, **kw)] = j
        nets = len(NET_CALLS)
        for h, (rws, _) in pool._rows.items():
            rows_of.setdefault(handles[h], list(rws))
        for h, out in pool.step().items():
            got[handles[h]] = out
        for h, (rws, _) in pool._rows.items():
            rows_of.setdefault(handles[h], list(rws))
        assert NET_CALLS[nets:] == [48], "a tick is ONE network call on the whole slab"
        tick += 1
    assert sorted(got) == list(range(len(reqs)))
    owners = {}
    for j in sorted(rows_of):
        for r in rows_of[j]:
            owners.setdefault(r, []).append(j)
    assert any(len(js) > 1 and sum(used[j][1][2] != 0 for j in js) > 1 for js in owners.values()), "no row reused under a momentum"
    for j, (_, kw, b, _, _) in enumerate(reqs):
        s, par = used[j]
        alone = _solver(dtype, s, par, *[c.expand(b, -1) for c in conds[j]])
        want = alone.sample(xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, (j, kw)
        assert torch.equal(got[j], want), (j, kw, b, s, par)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_steady_tick_of_apg_rows_is_one_network_call_one_launch_and_one_copy(dtype):
    dpm = _solver(dtype, 7.5, (0.0, 15.0, -0.5))
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [2.0 * torch.randn(1 + 2 * (j % 2), 4, 64, 64, generator=g, device=DEV).to(dtype) for j in range(10)]      # 20 rows
    pool = dpm.request_pool(slots=24, apg=True)
    own = lambda j: dict(guidance_scale=SCALES[j % 3], apg=(0.5, 0.0, 0.0)) if j % 2 else {}     # rows with and without a momentum
    hs = [pool.submit(x, steps=6 + j % 3, order=1 + j % 3, **own(j)) for j, x in enumerate(xs)]
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    names = []
    for _ in range(2):
        assert len(pool) == 10
        nets = len(NET_CALLS)
        # (names_of runs its function twice: once outside the profile)
        names.append(names_of(lambda: done.update(pool.step())))
        assert NET_CALLS[nets:] == [48, 48]
    assert all(len(n) == 1 and "stage_apg_kernel_table" in n[0] for n in names), names
    assert pool.copies == 6                                 # one per tick, and the admitting tick's time vector
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        alone = _solver(dtype, SCALES[j % 3], (0.5, 0.0, 0.0)) if j % 2 else dpm
        assert torch.equal(done[h], alone.sample(x, steps=6 + j % 3, order=1 + j % 3)), j
