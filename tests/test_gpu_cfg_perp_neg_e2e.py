"""Perp-Neg guidance end to end on the GPU: sample() through dpm_solver_amd.cfg_perp_neg with a small convolutional stand-in
network at [3,4,16,16], 6 steps.  The network's outputs of the run under test are RECORDED and replayed to the reference run, so
both see the same tensors (a network re-evaluated on a state that differs in the last bit may round an output element the other
way, which is a property of the network, not of the solver):
  * against a float64 statement of the same trajectory -- projection, blend and conversion written out in torch float64 here
    (perp_noise_float64: nothing of the wrapper), inside the engine's double-precision sampler -- for multistep and singlestep
    of order 1 to 3, both algorithm types, fp32 / fp16 / bf16 networks over an fp32 state, at the project's parity bar, 1e-5 of
    the tensor's scale (README, "parity with the reference").  Measured maxima: profiles/r32_cfg_perp_neg.md;
  * half states against the engine's host code on the numpy double (tests/perp_double.py) fed the same outputs, bit for bit;
  * a channels_last network, a captured run (auto_capture) and a RequestPool without slots: the bits of sample().
Run on an MI355X:  pytest -m gpu"""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import perp_double as PP
from engine_cases import make_schedule

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (3, 4, 16, 16)
SCALE, NEG_SCALE = 7.5, 1.5
RUNS = [(m, o, a) for m in ("multistep", "singlestep") for o in (1, 2, 3) for a in ("dpmsolver++", "dpmsolver")]
RUN_IDS = ["%s-%d-%s" % r for r in RUNS]
NET_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NET_IDS = ["fp32", "fp16", "bf16"]


def conv_net(dtype, record=None):
    """a 3x3 convolution over the channels plus terms in t and the condition, not linear in the condition -- the negative
    direction is neither parallel nor perpendicular to the positive one; answers in `dtype`"""
    w = (torch.randn(4, 4, 3, 3, generator=torch.Generator().manual_seed(3)) * 0.15)

    def net(x, t, c):
        cc = c.reshape(-1, 1, 1, 1).float()
        y = torch.nn.functional.conv2d(x.float(), w.to(x.device), padding=1) + 0.3 * torch.tanh(x.float())
        # (gains chosen so that the guided output at scale 7.5 stays of the order of x: the trajectories are finite in fp16)
        y = y * (0.3 + 0.03 * cc) + 0.05 * cc * torch.cos(2.0 * x.float() * cc) + 0.0002 * t.reshape(-1, 1, 1, 1).float()
        out = y.to(dtype)
        if record is not None:
            record.append(out)
        return out
    return net


def pointwise_net(x, t, c):
    cc = c.reshape(-1, 1, 1, 1)
    return (torch.tanh(x * 0.7) * (0.3 + 0.03 * cc) + 0.05 * x + 0.05 * cc * torch.cos(2.0 * x * cc)).to(x.dtype)


def wrap(net, ns, model_type, device, on=True):
    c = torch.tensor([1.0, 2.0, 3.0], device=device)
    fn = D.model_wrapper(net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=SCALE, condition=c,
                         unconditional_condition=c * 0)
    return D.cfg_perp_neg(fn, -0.5 * c, NEG_SCALE) if on else fn


def replay(outs, device, dtype=None):
    it = iter(outs)

    def net(x, t, c):
        o = next(it).to(device)
        return o if dtype is None else o.to(dtype)
    return net


def x_T(dtype=torch.float32):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(11)).to(dtype)


def perp_noise_float64(outs, ns, model_type):
    """model_fn(x, t[B]) -> noise in torch float64 from the recorded [3B, ...] outputs (empty, positive, negative): the
    projection and the blend on the raw outputs, then the conversion, every operation in double"""
    it = iter(outs)

    def fn(x, t):
        o_u, o_c, o_n = next(it).to(x.device).double().chunk(3)
        d0, d2 = o_c - o_u, o_n - o_u
        a = (d2 * d0).sum(dim=(1, 2, 3), keepdim=True) / (d0 * d0).sum(dim=(1, 2, 3), keepdim=True)
        gd = o_u + SCALE * (d0 - NEG_SCALE * (d2 - a * d0))
        if model_type == "v":
            t64 = t.double().reshape(-1)
            al = ns.marginal_alpha(t64).reshape(-1, 1, 1, 1).double()
            sg = ns.marginal_std(t64).reshape(-1, 1, 1, 1).double()
            gd = al * gd + sg * x.double()
        return gd
    return fn


@gpu
@pytest.mark.parametrize("ndt", NET_DTYPES, ids=NET_IDS)
@pytest.mark.parametrize("method,order,algo", RUNS, ids=RUN_IDS)
def test_sample_against_a_float64_statement(method, order, algo, ndt):
    """within the project's parity bar, 1e-5 of the tensor's scale.  Measured on an MI355X (maxima over the twelve runs): see
    profiles/r32_cfg_perp_neg.md, section 4."""
    ns = make_schedule("sd")
    kw = dict(steps=6, order=order, method=method)
    for model_type in ("noise", "v"):
        rec = []
        x = x_T().to(DEV)
        got = D.DPM_Solver(wrap(conv_net(ndt, rec), ns, model_type, DEV), ns, algorithm_type=algo).sample(x, **kw)
        assert got.dtype is torch.float32 and len(rec) >= 6 and all(r.shape[0] == 3 * SHAPE[0] for r in rec)
        want = D.DPM_Solver(perp_noise_float64(rec, ns, model_type), ns, algorithm_type=algo).sample(x.double(), **kw)
        assert want.dtype is torch.float64
        err = float((got.double() - want).abs().max() / want.abs().max())
        print("cfg_perp_neg %s-%d %s %s %s vs float64: %.3g of the scale" % (method, order, algo, model_type, ndt, err))
        assert err <= 1e-5
        # the negative prompt is not a no-op here: classifier-free guidance on the first two thirds gives another result
        two = [r[:2 * SHAPE[0]] for r in rec]
        plain = D.DPM_Solver(wrap(replay(two, DEV), ns, model_type, DEV, on=False), ns, algorithm_type=algo).sample(x, **kw)
        assert float((plain - got).abs().max() / got.abs().max()) > 1e-3


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("method,order,algo", [("multistep", 2, "dpmsolver++"), ("multistep", 3, "dpmsolver"),
                                               ("singlestep", 3, "dpmsolver++"), ("singlestep", 2, "dpmsolver")])
def test_half_states_are_the_double_bit_for_bit(method, order, algo, model_type, sdt, monkeypatch):
    """sample(), return_intermediate state by state and sample_requests on a half state, against the engine's host code on the
    numpy double fed the recorded outputs (whose inputs the double asserts decidable before it computes)"""
    ns = make_schedule("sd")
    kw = dict(steps=6, order=order, method=method)
    rec = []
    x = x_T(sdt)
    mk = lambda net, dev: D.DPM_Solver(wrap(net, ns, model_type, dev), ns, algorithm_type=algo, state_dtype=sdt)
    got = mk(conv_net(sdt, rec), DEV).sample(x.to(DEV), **kw)
    assert got.dtype is sdt and len(rec) >= 6 and bool(torch.isfinite(got).all())
    with monkeypatch.context() as m:
        PP.install_perp_double(m, S, D)
        want = mk(replay(rec, "cpu"), "cpu").sample(x, **kw)
        wi = mk(replay(rec, "cpu"), "cpu").sample(x, return_intermediate=True, **kw)[1]
    assert torch.equal(got.cpu(), want)
    gi = mk(replay(rec, DEV), DEV).sample(x.to(DEV), return_intermediate=True, **kw)[1]      # the general loop, state by state
    assert len(gi) == len(wi) and all(torch.equal(a.cpu(), b) for a, b in zip(gi, wi))
    outs = mk(replay([r for r in rec for _ in range(2)], DEV), DEV).sample_requests([x.to(DEV), x.to(DEV)], **kw)
    assert torch.equal(outs[0], got) and torch.equal(outs[1], got)


@gpu
def test_wrapper_call_is_the_one_stage_denoise_launch():
    """WrappedModel.__call__ -- the torch statement of the contract -- against noise_prediction_fn, one DENOISE launch of
    stage_perp_kernel.  Both take the sums in double, in different orders; a is the same fp32 value unless its double sits on a
    rounding boundary, so an fp32 noise network gives equal bits or -- where one of three a's moved by an ulp -- 1e-6 of the
    scale; a v network adds the conversion's scalars, formed on either side: 1e-5."""
    ns = make_schedule("sd")
    x = x_T().to(DEV)
    t = torch.full((SHAPE[0],), 0.6, device=DEV)
    # (a half noise network over an fp32 x gives a half noise_prediction_fn, the reference's promotion: not comparable here)
    for ndt, mt in [(torch.float32, "noise"), (torch.float32, "v"), (torch.float16, "v"), (torch.bfloat16, "v")]:
        fn = wrap(conv_net(ndt), ns, mt, DEV)
        a, b = fn(x, t), D.DPM_Solver(fn, ns, algorithm_type="dpmsolver").noise_prediction_fn(x, torch.tensor([0.6], device=DEV))
        assert a.dtype is torch.float32 and b.dtype is torch.float32
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        print("cfg_perp_neg __call__ vs DENOISE launch, %s %s network: %.3g of the scale" % (ndt, mt, err))
        assert err <= (1e-6 if mt == "noise" else 1e-5)
    off = wrap(conv_net(torch.float32), ns, "noise", DEV, on=False)
    fn = wrap(conv_net(torch.float32), ns, "noise", DEV)
    assert float((off(x, t) - fn(x, t)).abs().max() / fn(x, t).abs().max()) > 1e-3       # the negative prompt is not a no-op


@gpu
@pytest.mark.parametrize("sdt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_a_channels_last_network_gives_the_same_bits(sdt):
    ns = make_schedule("sd")
    kw = dict(steps=6, order=2)
    skw = dict(state_dtype=sdt) if sdt is torch.float16 else {}
    x = x_T(sdt).to(DEV)
    nhwc = lambda xx, t, c: pointwise_net(xx, t, c).contiguous(memory_format=torch.channels_last)
    want = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV), ns, **skw).sample(x, **kw)
    got = D.DPM_Solver(wrap(nhwc, ns, "v", DEV), ns, **skw).sample(x.contiguous(memory_format=torch.channels_last), **kw)
    assert got.shape == want.shape and torch.equal(got.contiguous(), want)


@gpu
@pytest.mark.parametrize("sdt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_a_captured_run_equals_the_eager_bits(sdt):
    """auto_capture: the second call of sample() on a shape replays a graph; capture() the same -- the eager run's bits, also on
    another input"""
    ns = make_schedule("sd")
    kw = dict(steps=6, order=2)
    skw = dict(state_dtype=sdt) if sdt is torch.float16 else {}
    x = x_T(sdt).to(DEV)
    x2 = (x_T(sdt).float() * 0.5 + 0.1).to(sdt).to(DEV)
    eager = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV), ns, **skw)
    want, want2 = eager.sample(x, **kw), eager.sample(x2, **kw)
    auto = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV), ns, **skw)
    auto.auto_capture = True
    for _ in range(3):
        assert torch.equal(auto.sample(x, **kw), want)
    assert torch.equal(auto.sample(x2, **kw), want2)
    g = eager.capture(x, **kw)
    assert torch.equal(g(x), want) and torch.equal(g(x2), want2)
    off = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV, on=False), ns, **skw).sample(x, **kw)
    assert not torch.equal(want, off)


@gpu
def test_a_request_pool_without_slots_and_sample_requests_give_the_bits_of_sample():
    ns = make_schedule("sd")
    dpm = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV), ns)
    xs = [x_T().to(DEV), (x_T() * 0.7 + 0.2).to(DEV)]
    kw = dict(steps=6, order=2, denoise_to_zero=True)
    want = [dpm.sample(x, **kw) for x in xs]
    outs = dpm.sample_requests(xs, **kw)
    assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])
    pool = dpm.request_pool()
    hs = [pool.submit(xs[0], **kw)]
    done = dict(pool.step())
    hs.append(pool.submit(xs[1], **kw))                                       # ... admitted one stage late: other positions
    for _ in range(10):
        done.update(pool.step())
    assert set(done) == set(hs) and all(torch.equal(done[h], w) for h, w in zip(hs, want))
    with pytest.raises(NotImplementedError, match="a follow-up"):
        dpm.request_pool(slots=8, pair=True)
    # a double state projects and blends the three outputs in torch, in double, and runs an unguided double stage.  The network
    # is evaluated in double there and in fp32 above, on states that drift apart by fp32 roundings over seven evaluations: the
    # two runs agree to 1e-4 of the scale (on the CPU double of this case they differ by 8.5e-6), far from the 0.58 the
    # negative prompt moves this result by -- a check that the path runs and means the same, not a parity bar
    d = dpm.sample(xs[0].double(), **kw)
    assert d.dtype is torch.float64 and float((d - want[0].double()).abs().max() / d.abs().max()) <= 1e-4
