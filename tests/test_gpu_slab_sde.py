"""An SDE slab pool (DPM_Solver.request_pool(slots=S, sde=True)) on the MI355X: 30 staggered requests -- SDE-DPM-Solver++, 2M-style
multistep and UniPC, 1..3 samples each -- in 40 rows of sample shape [4, 8, 8], fp32 and fp16, unconditional and
classifier-free, with an elementwise network of the row's state, time and condition.  Every SDE result must equal
sample_sde(x, seed=...) on the request alone bit for bit, whichever rows its samples landed in; the others equal sample() /
sample_unipc(); and a tick of 24 SDE rows is ONE stage_kernel_table_noise launch.
Run on an MI355X:  pytest -m gpu
"""
import pytest
import torch

from dpm_solver_amd.slab import SlabPool
from test_gpu_slab_pool import _solver
from test_gpu_unipc_pool import _stage_kernels

gpu = pytest.mark.gpu
DEV = "cuda:0"


def scenario(n=30):
    """(tick of submission, kind, kwargs, b): four requests per tick, kinds in rotation, steps 4..9; the last, a lone SDE sample,
    outlives the others"""
    out = []
    for j in range(n):
        steps, b = 4 + j % 6, 1 + j % 3
        kind = ("sde", "2m", "sde", "unipc")[j % 4]
        if kind == "sde":
            kw = dict(steps=steps, order=1 + (j // 2) % 2, solver_type=("dpmsolver", "taylor")[j % 8 == 0],
                      denoise_to_zero=(j % 6 == 0), seed=(0x9E3779B97F4A7C15 * (j + 1)) % (1 << 64))
        elif kind == "2m":
            kw = dict(steps=steps, order=1 + (j // 4) % 3, skip_type=("time_uniform", "logSNR")[j % 8 == 1])
        else:
            kw = dict(steps=steps, order=2, variant=("bh2", "bh1")[j % 8 == 3])
        out.append((j // 4, kind, kw, b))
    out.append((n // 4, "sde", dict(steps=16, order=2, seed=7), 1))
    return out


def run_pool(pool, reqs, xs, on_tick=None):
    handles, got, tick = {}, {}, 0
    while tick <= max(r[0] for r in reqs) or pool:
        for j, (t, kind, kw, b) in enumerate(reqs):
            if t == tick:
                sub = pool.submit_unipc if kind == "unipc" else pool.submit
                handles[sub(xs[j], sde=True, **kw) if kind == "sde" else sub(xs[j], **kw)] = j
        if on_tick:
            on_tick(pool)
        for h, out in pool.step().items():
            got[handles[h]] = out
        tick += 1
    return got


def sde_rows(pool):
    """rows that will advance by an SDE stage at the next step (after its admissions)"""
    pool._admit()
    return int(((pool._req >= 0) & (pool._optp != 0)).sum()), int((pool._req >= 0).sum())


@gpu
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_staggered_sde_slab_pool_equals_every_request_alone(dtype, cfg):
    reqs = scenario()
    g = torch.Generator().manual_seed(209)
    xs = [torch.randn(b, 4, 8, 8, generator=g).to(DEV).to(dtype) for _, _, _, b in reqs]
    dpm = _solver(cfg, dtype)
    pool = dpm.request_pool(slots=40, sde=True)
    assert isinstance(pool, SlabPool)
    counts = []
    got = run_pool(pool, reqs, xs, lambda p: counts.append(sde_rows(p)) if p._like is not None else None)
    assert sorted(got) == list(range(len(reqs)))
    # ticks of more than 16 rows and of fewer, SDE rows above 16, below, and a lone one
    assert max(a for _, a in counts) > 16 and min(a for _, a in counts if a) < 16
    assert max(s for s, _ in counts) > 16 and any(1 < s < 16 for s, _ in counts) and any(s == 1 for s, _ in counts)
    for j, (_, kind, kw, b) in enumerate(reqs):
        want = {"sde": dpm.sample_sde, "2m": dpm.sample, "unipc": dpm.sample_unipc}[kind](xs[j], **kw)
        assert got[j].shape == xs[j].shape and got[j].dtype == want.dtype == dtype, (j, kind, kw)
        assert torch.equal(got[j], want), (j, kind, kw, b)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_tick_of_24_sde_rows_is_one_table_noise_launch(dtype):
    dpm = _solver(False, dtype)
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [torch.randn(1 + j % 2, 4, 8, 8, generator=g, device=DEV).to(dtype) for j in range(16)]      # 24 rows
    pool = dpm.request_pool(slots=40, sde=True)
    hs = [pool.submit(x, steps=6 + j % 3, order=2, sde=True, seed=50 + j) for j, x in enumerate(xs)]
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    names = []
    for _ in range(4):
        assert len(pool) == 16
        names.append(_stage_kernels(lambda: done.update(pool.step())))
    assert all(len(n) == 1 and "stage_kernel_table_noise" in n[0] for n in names), names
    assert pool.copies == 6                                 # one per tick, and the admitting tick's time vector
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        assert torch.equal(done[h], dpm.sample_sde(x, steps=6 + j % 3, order=2, seed=50 + j)), j
