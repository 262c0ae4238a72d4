"""A request pool of mixed shapes (DPM_Solver.request_pool(mixed_shapes=True)), without a GPU: the pool's host code on the
numpy doubles -- kernel_double.py, unipc_double.py, sde_double.py -- behind a double of dpm_stage_launch_multi that honours
per-request stage records.  Requests of six shapes (one of them no multiple of 8 elements), admitted at staggered ticks as
second-order and third-order multistep, UniPC and SDE requests, must each equal the request sampled alone, bit for bit; every
tick is ONE multi-request call whose options carry dpm_launch_opts.fuse_shapes.  The default pool keeps its shape error, a
mixed pool its dtype error, and the C ABI reports version 207 with a dpm_launch_opts of unchanged size."""
import ctypes

import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import kernel_double as KD
import sde_double as SD  # noqa: F401  (installed through test_unipc_pool_host.launch_raw)
import unipc_double as UD
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule
from test_unipc_pool_host import launch_raw

SHAPES = [(1, 4, 8, 8), (2, 4, 16, 16), (3, 4, 16, 16), (2, 4, 32, 32), (1, 3, 24, 24), (1, 3, 5, 5)]
CALLS = []          # (requests, per_request_stages, fuse_shapes, distinct element counts) of every multi-request call


def launch_multi(st, bufs, n_req, stream):
    o = bufs[0].opts.contents if bufs[0].opts else None
    per = o is not None and o.per_request_stages == 1
    CALLS.append((int(n_req), per, 0 if o is None else int(o.fuse_shapes), len({int(bufs[r].n) for r in range(int(n_req))})))
    for r in range(int(n_req)):
        rc = launch_raw(KD._Ref(st[r] if per else st._obj), KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


@pytest.fixture
def doubles(monkeypatch):
    UD.install_unipc_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi)
    CALLS.clear()


def _solver(cfg):
    ns = make_schedule("sd")
    if cfg:
        def net(x, t, c):       # c = [uncond, cond], one entry per half of the [2B, ...] input, whatever B
            w = c.repeat_interleave(x.shape[0] // c.shape[0]).reshape(-1, 1, 1, 1)
            return torch.tanh(x * 0.7) * (0.5 + 0.1 * w)
        c = torch.ones(1)
        fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=3.0, condition=c,
                             unconditional_condition=c * 0)
    else:
        fn = D.model_wrapper(lambda x, t: torch.tanh(x * 0.7) + 0.01 * t.reshape(-1, 1, 1, 1), ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")


# (tick of admission, shape index, kind, kwargs): every shape twice, every kind on three shapes
MIX = [
    (0, 0, "2m", dict(steps=6, order=2)),
    (0, 1, "unipc", dict(steps=7)),
    (0, 2, "sde", dict(steps=5, seed=0xDEADBEEF12345)),
    (1, 3, "ms3", dict(steps=8, order=3)),
    (1, 4, "2m", dict(steps=4, order=2, skip_type="logSNR")),
    (2, 5, "unipc", dict(steps=5, variant="bh1")),
    (2, 0, "sde", dict(steps=6, seed=3)),
    (3, 1, "ms3", dict(steps=7, order=3, lower_order_final=False)),
    (3, 2, "2m", dict(steps=9, order=2)),
    (5, 3, "unipc", dict(steps=3, order=2)),
    (5, 4, "sde", dict(steps=4, seed=11, order=1)),
    (6, 5, "ms3", dict(steps=6, order=3)),
]
SUBMIT = {"2m": lambda p, x, kw: p.submit(x, **kw), "ms3": lambda p, x, kw: p.submit(x, **kw),
          "unipc": lambda p, x, kw: p.submit_unipc(x, **kw), "sde": lambda p, x, kw: p.submit(x, sde=True, **kw)}


def _alone(dpm, kind, x, kw):
    return {"2m": dpm.sample, "ms3": dpm.sample, "unipc": dpm.sample_unipc, "sde": dpm.sample_sde}[kind](x, **kw)


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
def test_staggered_pool_of_six_shapes_equals_every_request_alone(doubles, cfg):
    assert {s for _, s, _, _ in MIX} == set(range(len(SHAPES))) and {k for _, _, k, _ in MIX} == set(SUBMIT)
    dpm = _solver(cfg)
    g = torch.Generator().manual_seed(207)
    xs = [torch.randn(*SHAPES[s], generator=g) for _, s, _, _ in MIX]
    want = [_alone(dpm, k, x, kw) for x, (_, _, k, kw) in zip(xs, MIX)]
    CALLS.clear()
    pool = dpm.request_pool(mixed_shapes=True)
    handles, got, tick = {}, {}, 0
    while tick <= max(m[0] for m in MIX) or pool:
        for j, (t, _, k, kw) in enumerate(MIX):
            if t == tick:
                handles[SUBMIT[k](pool, xs[j], kw)] = j
        n_active, n_calls = len(pool), len(CALLS)
        for h, out in pool.step().items():
            got[handles[h]] = out
        if n_active:      # ONE multi-request call per tick: per-request records, fuse_shapes set
            assert [c[:3] for c in CALLS[n_calls:]] == [(n_active, True, 1)]
        tick += 1
    assert max(c[3] for c in CALLS) >= 5                                  # ticks really held many element counts at once
    assert sorted(got) == list(range(len(MIX)))
    for j, w in enumerate(want):
        assert got[j].shape == xs[j].shape == w.shape and got[j].dtype == w.dtype, MIX[j]
        assert torch.equal(got[j], w), MIX[j]
        assert got[j].data_ptr() != xs[j].data_ptr()


def test_the_default_pool_keeps_its_shape_error_and_its_options(doubles):
    dpm = _solver(False)
    pool = dpm.request_pool()
    x = torch.randn(*SHAPES[1])
    h = pool.submit(x, steps=3)
    with pytest.raises(ValueError, match=r"request pool: x of shape \(3, 4, 16, 16\), dtype torch.float32 on cpu does not match "
                                         r"the pool's \(2, 4, 16, 16\), torch.float32 on cpu"):
        pool.submit(torch.randn(*SHAPES[2]), steps=3)
    with pytest.raises(ValueError, match="does not match the pool's"):
        pool.submit_unipc(torch.randn(*SHAPES[0]), steps=3)
    done = {}
    while pool:
        done.update(pool.step())
    assert torch.equal(done[h], dpm.sample(x, steps=3))
    assert CALLS and all(c[1] and c[2] == 0 for c in CALLS)               # fuse_shapes stays 0
    assert dpm.request_pool(mixed_shapes=False)._mixed is False


def test_a_mixed_pool_still_fixes_dtype(doubles):
    dpm = _solver(False)
    pool = dpm.request_pool(mixed_shapes=True)
    pool.submit(torch.randn(*SHAPES[0]), steps=3)
    pool.submit(torch.randn(*SHAPES[3]), steps=3)                         # another shape: admitted
    with pytest.raises(ValueError, match=r"request pool: x of shape \(1, 4, 8, 8\), dtype torch.float64 on cpu does not match "
                                         r"the pool's"):
        pool.submit(torch.randn(*SHAPES[0]).double(), steps=3)
    with pytest.raises(ValueError, match="does not match the pool's"):
        pool.submit_unipc(torch.randn(*SHAPES[1]).half(), steps=3)
    with pytest.raises(ValueError, match="at least one dimension and one element"):
        pool.submit(torch.randn(()), steps=3)
    with pytest.raises(ValueError, match="at least one dimension and one element"):
        pool.submit(torch.randn(2, 0, 4), steps=3)
    assert len(pool) == 2


def test_abi_207_launch_opts_keeps_its_size():
    assert ctypes.sizeof(L.LaunchOpts) == 32 and L.lib.dpm_sizeof(5) == 32          # DPM_SIZEOF_LAUNCH_OPTS
    assert L.LaunchOpts.fuse_shapes.offset == 24 and L.LaunchOpts.reserved.offset == 28
    assert L.LaunchOpts.per_request_stages.offset == 12 and L.LaunchOpts.noise_seed_lo.offset == 16
    assert L.lib.dpm_version() >= 207
    assert L.LaunchOpts().fuse_shapes == 0
