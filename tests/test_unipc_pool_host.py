"""UniPC requests in the request pool (RequestPool.submit_unipc), without a GPU: the pool's host code on the numpy doubles --
unipc_double.py (the DPM_FORM_UNIPC stage), sde_double.py (the noise stage) and kernel_double.py (everything else) behind a
double of dpm_stage_launch_multi that honours dpm_launch_opts.per_request_stages.  Every result must equal the request's own
sample_unipc / sample / sample_sde call bit for bit, whatever else was in flight, and every tick is ONE multi-request call."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import kernel_double as KD
import sde_double as SD
import unipc_double as UD
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule

CALLS = []


def launch_raw(st_ref, b_ref, stream):
    """dpm_stage_launch: UniPC records on unipc_double, SDE records on sde_double, the rest on kernel_double"""
    st = st_ref._obj
    if st.form == L.FORM_UNIPC:
        return UD.launch_raw_double(st_ref, b_ref, stream)
    if st.flags & L.F_NOISE:
        return SD.launch_raw_noise_double(st_ref, b_ref, stream)
    return KD.launch_raw_double(st_ref, b_ref, stream)


def launch_multi_per_request(st, bufs, n_req, stream):
    """dpm_stage_launch_multi: with bs[0].opts->per_request_stages == 1, request r is advanced by st[r]"""
    per = bool(bufs[0].opts) and bufs[0].opts.contents.per_request_stages == 1
    CALLS.append((int(n_req), per))
    for r in range(int(n_req)):
        rc = launch_raw(KD._Ref(st[r] if per else st._obj), KD._Ref(bufs[r]), stream)
        if rc:
            return rc
    return 0


@pytest.fixture
def doubles(monkeypatch):
    UD.install_unipc_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw)
    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi_per_request)
    CALLS.clear()


def _solver(cfg=False, model_type="noise", **kw):
    ns = make_schedule("sd")
    if cfg:
        def net(x, t, c):
            return torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]])
        c = torch.ones(2)
        fn = D.model_wrapper(net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=3.0,
                             condition=c, unconditional_condition=c * 0)
    else:
        def net(x, t):
            return torch.tanh(x * 0.7) + 0.01 * t.reshape(-1, 1, 1, 1)
        fn = D.model_wrapper(net, ns, model_type=model_type)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", **kw)


def _xs(R, shape=(2, 3, 8, 8), seed=7, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=g).to(dtype) for _ in range(R)]


def _drain(pool, done=None):
    done = {} if done is None else done
    while pool:
        done.update(pool.step())
    return done


# (tick of admission, sample_unipc() kwargs): the smallest legal plans (one LIN1 stage; LIN1 + one first-order UniPC stage),
# both orders and variants, every skip type, denoise_to_zero, lower_order_final off (a second-order predictor to the end)
MIX = [
    (0, dict(steps=8)),
    (0, dict(steps=2, order=2)),
    (1, dict(steps=1, order=1)),
    (1, dict(steps=6, order=1, variant="bh1")),
    (2, dict(steps=7, variant="bh1", skip_type="logSNR")),
    (3, dict(steps=5, denoise_to_zero=True, skip_type="time_quadratic")),
    (3, dict(steps=9, lower_order_final=False)),
    (5, dict(steps=3, order=2, denoise_to_zero=True)),
    (6, dict(steps=12, skip_type="logSNR")),
    (11, dict(steps=4, order=1)),
]


@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
def test_staggered_unipc_pool_equals_sample_unipc(doubles, cfg):
    dpm = _solver(cfg)
    xs = _xs(len(MIX))
    want = [dpm.sample_unipc(x, **kw) for x, (_, kw) in zip(xs, MIX)]
    CALLS.clear()
    pool = dpm.request_pool()
    handles, got, tick = {}, {}, 0
    while tick <= max(t for t, _ in MIX) or pool:
        for j, (t, kw) in enumerate(MIX):
            if t == tick:
                handles[pool.submit_unipc(xs[j], **kw)] = j
        n_active, n_calls = len(pool), len(CALLS)
        for h, out in pool.step().items():
            got[handles[h]] = out
        if n_active:
            assert CALLS[n_calls:] == [(n_active, True)]      # ONE multi-request call per tick, with per-request records
        tick += 1
    assert sorted(got) == list(range(len(MIX)))
    for j, w in enumerate(want):
        assert got[j].dtype == w.dtype and torch.equal(got[j], w), MIX[j]
        assert got[j].data_ptr() != xs[j].data_ptr()


def test_staggered_half_precision_states(doubles):
    ns = D.NoiseScheduleVP("linear")             # (a half state stays half on a continuous schedule with a noise network)
    net = lambda x, t: (0.5 * x.float() + 0.1 * torch.sin(x.float())).to(x.dtype)
    dpm = D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++")
    xs = _xs(3, dtype=torch.float16)
    kws = [dict(steps=6), dict(steps=4, variant="bh1"), dict(steps=5, order=1)]
    pool = dpm.request_pool()
    hs = []
    for x, kw in zip(xs, kws):
        hs.append(pool.submit_unipc(x, **kw))
        pool.step()
    done = _drain(pool)
    for h, x, kw in zip(hs, xs, kws):
        w = dpm.sample_unipc(x, **kw)
        assert done[h].dtype == w.dtype == torch.float16 and torch.equal(done[h], w)
    with pytest.raises(NotImplementedError, match="denoise_to_zero with a half-precision state"):
        pool.submit_unipc(xs[0], steps=4, denoise_to_zero=True)


def test_mixed_pool_of_unipc_2m_singlestep_and_sde(doubles):
    dpm = _solver()
    xs = _xs(5, seed=3)
    pool = dpm.request_pool()
    h_uni = pool.submit_unipc(xs[0], steps=7)
    h_2m = pool.submit(xs[1], steps=6, order=2)
    pool.step()
    h_ss = pool.submit(xs[2], steps=6, order=3, method="singlestep")
    h_sde = pool.submit(xs[3], steps=5, sde=True, seed=0xDEADBEEF12345)
    pool.step()
    h_uni2 = pool.submit_unipc(xs[4], steps=5, variant="bh1")
    done = _drain(pool)
    assert all(c[1] for c in CALLS)
    assert torch.equal(done[h_uni], dpm.sample_unipc(xs[0], steps=7))
    assert torch.equal(done[h_2m], dpm.sample(xs[1], steps=6, order=2))
    assert torch.equal(done[h_ss], dpm.sample(xs[2], steps=6, order=3, method="singlestep"))
    assert torch.equal(done[h_sde], dpm.sample_sde(xs[3], steps=5, seed=0xDEADBEEF12345))
    assert torch.equal(done[h_uni2], dpm.sample_unipc(xs[4], steps=5, variant="bh1"))
    assert not torch.equal(done[h_uni], dpm.sample(xs[0], steps=7))          # (the corrector is there)


def test_corrector_off_is_the_multistep_plan(doubles):
    dpm = _solver()
    x, y = _xs(2, seed=9)
    pool = dpm.request_pool()
    h = pool.submit_unipc(x, steps=6, corrector=False)
    h2 = pool.submit_unipc(y, steps=6)
    done = _drain(pool)
    assert torch.equal(done[h], dpm.sample(x, steps=6, order=2, method="multistep", solver_type="dpmsolver"))
    assert torch.equal(done[h], dpm.sample_unipc(x, steps=6, corrector=False))
    assert torch.equal(done[h2], dpm.sample_unipc(y, steps=6))
    with pytest.raises(NotImplementedError, match="corrector=False with variant='bh1'"):
        pool.submit_unipc(x, corrector=False, variant="bh1")


def test_errors_come_before_any_device_work():
    """no double installed: a CPU tensor, so any device work -- and an admission -- would raise RuntimeError"""
    ns = make_schedule("sd")
    x = torch.zeros(2, 4, 8, 8)
    net = lambda x, t: x
    pool = D.DPM_Solver(net, ns, algorithm_type="dpmsolver++").request_pool()
    with pytest.raises(NotImplementedError, match="noise-prediction"):
        D.DPM_Solver(net, ns, algorithm_type="dpmsolver").request_pool().submit_unipc(x)
    with pytest.raises(NotImplementedError, match="thresholding"):
        D.DPM_Solver(net, ns, correcting_x0_fn="dynamic_thresholding").request_pool().submit_unipc(x)
    with pytest.raises(NotImplementedError, match="callable"):
        D.DPM_Solver(net, ns, correcting_x0_fn=lambda x0, t: x0).request_pool().submit_unipc(x)
    with pytest.raises(NotImplementedError, match="correcting_xt_fn"):
        D.DPM_Solver(net, ns, correcting_xt_fn=lambda x, t, step: x).request_pool().submit_unipc(x)
    with pytest.raises(ValueError, match="'order' must be 1 or 2.*follow-up"):
        pool.submit_unipc(x, order=3)
    with pytest.raises(ValueError, match="'variant' must be either 'bh1' or 'bh2'"):
        pool.submit_unipc(x, variant="vary_coeff")
    with pytest.raises(ValueError, match="'order' must be 1 or 2"):      # the solver's checks come first, in sample_unipc's order
        pool.submit_unipc(x.double(), order=0, variant="bh3", t_end=-1.0)
    with pytest.raises(ValueError, match="variant"):
        pool.submit_unipc(x.double(), variant="bh3", t_end=-1.0)
    with pytest.raises(AssertionError, match="Time range"):
        pool.submit_unipc(x.double(), t_end=-1.0)
    with pytest.raises(NotImplementedError, match="double"):
        pool.submit_unipc(x.double(), corrector=False, variant="bh1")
    with pytest.raises(NotImplementedError, match="corrector=False with variant='bh1'"):
        pool.submit_unipc(x, corrector=False, variant="bh1")
    with pytest.raises(ValueError, match="skip_type"):
        pool.submit_unipc(x, skip_type="nope")
    with pytest.raises(AssertionError):
        pool.submit_unipc(x, steps=1, order=2)
    with pytest.raises(TypeError):
        pool.submit_unipc(x, return_intermediate=True)
    with pytest.raises(NotImplementedError, match="UniPC.*submit_unipc|submit_unipc.*UniPC"):
        pool.submit(x, unipc="bh2")
    for bad in (None, [x], x.numpy()):            # a non-tensor: the solver's checks first, then the device requirement
        with pytest.raises(ValueError, match="variant"):
            pool.submit_unipc(bad, variant="bh3")
        with pytest.raises(RuntimeError, match="got a <class .*no CPU fallback"):
            pool.submit_unipc(bad, skip_type="nope")
        with pytest.raises(RuntimeError, match="got a <class .*no CPU fallback"):
            pool.submit_unipc(bad, corrector=False)
    for kw in (dict(), dict(corrector=False)):                           # ... and the checks pass: the device is required
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pool.submit_unipc(x, **kw)
    assert not pool and pool._like is None


def test_the_pools_own_errors(doubles):
    dpm = _solver()
    x = _xs(1)[0]
    with pytest.raises(ValueError, match="at least one dimension"):
        dpm.request_pool().submit_unipc(torch.randn(()))
    for bad in (None, [x], x.numpy()):            # a non-tensor, where the device requirement is the double's: the pool's error
        with pytest.raises(ValueError, match="request pool: x must be a tensor"):
            dpm.request_pool().submit_unipc(bad)
        with pytest.raises(ValueError, match="request pool: x must be a tensor"):
            dpm.request_pool().submit_unipc(bad, corrector=False, skip_type="nope")
    pool = dpm.request_pool()
    pool.submit_unipc(x, steps=4)
    with pytest.raises(ValueError, match="shape"):
        pool.submit_unipc(torch.randn(1, 3, 8, 8))
    with pytest.raises(ValueError, match="dtype"):
        pool.submit_unipc(x.half())
    with pytest.raises(ValueError, match="does not match the pool's"):
        pool.submit_unipc(x.to("meta"))
    with pytest.raises(ValueError, match="skip_type"):                  # sample_unipc's errors first
        pool.submit_unipc(torch.randn(1, 3, 8, 8), skip_type="nope")
    assert len(pool) == 1
    _drain(pool)


def test_a_finished_requests_scratch_is_taken_up_by_the_next(doubles):
    dpm = _solver()
    x1, x2 = _xs(2, seed=1)
    pool = dpm.request_pool()
    h1 = pool.submit_unipc(x1, steps=4)
    done = _drain(pool)
    fr = pool._free and next(iter(pool._free.values()))[0]
    h2 = pool.submit_unipc(x2, steps=4)
    pool.step()
    assert pool._active[h2].fr is fr                 # the finished request's launch records and scratch
    h3 = pool.submit(x1, steps=4, order=2)           # another plan: another key, records of its own
    pool.step()
    assert pool._active[h3].fr is not fr
    _drain(pool, done)
    assert torch.equal(done[h1], dpm.sample_unipc(x1, steps=4))
    assert torch.equal(done[h2], dpm.sample_unipc(x2, steps=4))
    assert torch.equal(done[h3], dpm.sample(x1, steps=4, order=2))
    assert done[h1].data_ptr() != done[h2].data_ptr()


def test_version():
    assert L.lib.dpm_version() >= 206
