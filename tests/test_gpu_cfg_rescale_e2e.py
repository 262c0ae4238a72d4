"""Guidance rescale end to end on the GPU: sample() through dpm_solver_amd.cfg_rescale with a small convolutional stand-in
network at [2,4,16,16], 6 steps.  The network's outputs of the run under test are RECORDED and replayed to the reference run, so
both see the same half-precision tensors (a network re-evaluated on a state that differs in the last bit may round an output
element the other way, which is a property of the network, not of the solver):
  * an fp32 state with an fp16 network against a float64 loop whose model function is WrappedModel.__call__ (torch,
    statistics in float64), at 1e-5 of the scale: for every method the engine's double-precision path on
    x.double(), and for multistep order 2 also a 2M loop written out in plain torch float64 (torch_2m_float64), which shares
    neither planner nor kernels with the run under test;
    measured on an MI355X: 5.8e-8 .. 1.3e-7 over the six cases;
  * an fp16 state against the engine's host code on the numpy double (tests/rescale_double.py), stage by stage, bit for bit.
Run on an MI355X:  pytest -m gpu"""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import rescale_double as RD
from engine_cases import make_schedule

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (2, 4, 16, 16)
RUNS = [("multistep", 2), ("multistep", 3), ("singlestep", 3)]


def conv_net(dtype, record=None):
    """a 3x3 convolution over the channels plus terms in t and the condition; answers in `dtype`"""
    w = (torch.randn(4, 4, 3, 3, generator=torch.Generator().manual_seed(3)) * 0.15)

    def net(x, t, c):
        y = torch.nn.functional.conv2d(x.float(), w.to(x.device), padding=1) + 0.3 * torch.tanh(x.float())
        y = y * (0.6 + 0.2 * c.reshape(-1, 1, 1, 1).float()) + 0.0002 * t.reshape(-1, 1, 1, 1).float()
        out = y.to(dtype)
        if record is not None:
            record.append(out)
        return out
    return net


def pointwise_net(x, t, c):
    return (torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)) + 0.05 * x).to(x.dtype)


def wrap(net, ns, model_type, device, phi=0.7):
    c = torch.tensor([1.0, 2.0], device=device)
    fn = D.model_wrapper(net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=7.5, condition=c,
                         unconditional_condition=c * 0)
    return fn if phi is None else D.cfg_rescale(fn, phi)


def replay(outs, device, dtype=None):
    it = iter(outs)

    def net(x, t, c):
        o = next(it).to(device)
        return o if dtype is None else o.to(dtype)
    return net


def x_T(dtype=torch.float32):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(11)).to(dtype)


@gpu
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("method,order", RUNS)
def test_fp32_state_fp16_network_against_a_float64_loop(method, order, model_type):
    ns = make_schedule("sd")
    algo = "dpmsolver" if (order == 3 and model_type == "noise") else "dpmsolver++"
    kw = dict(steps=6, order=order, method=method)
    rec = []
    x = x_T().to(DEV)
    got = D.DPM_Solver(wrap(conv_net(torch.float16, rec), ns, model_type, DEV), ns, algorithm_type=algo).sample(x, **kw)
    assert got.dtype is torch.float32 and len(rec) == 6
    ref_fn = wrap(replay(rec, DEV), ns, model_type, DEV)
    want = D.DPM_Solver(lambda xx, t: ref_fn(xx, t), ns, algorithm_type=algo).sample(x.double(), **kw)
    assert want.dtype is torch.float64
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("cfg_rescale %s-%d %s %s vs float64: %.3g of the scale" % (method, order, model_type, algo, err))
    assert err <= 1e-5
    # the rescale is not a no-op here: without it the same outputs give another result
    plain = D.DPM_Solver(wrap(replay(rec, DEV), ns, model_type, DEV, phi=None), ns, algorithm_type=algo).sample(x, **kw)
    assert float((plain - got).abs().max() / want.abs().max()) > 1e-3


def torch_2m_float64(model_fn, ns, x, steps):
    """DPM-Solver++(2M) written out in torch float64, independent of the engine's planner and kernels: the reference's
    multistep loop (ref :1171-1212) with time_uniform steps, lower_order_final, solver_type 'dpmsolver' (ref :547-592, :827-851).
    model_fn(x, t_continuous[B]) -> noise; the schedule's marginals are evaluated at double times."""
    dev, B = x.device, x.shape[0]
    ts = torch.linspace(ns.T, 1. / ns.total_N, steps + 1).double()                      # the reference's fp32 grid, exactly
    marg = lambda t: tuple(float(f(t.reshape(1))) for f in (ns.marginal_lambda, ns.marginal_alpha, ns.marginal_std))

    def x0_at(xx, t):                                                                   # data_prediction_fn, ref :433-442
        _, a, s = marg(t)
        return (xx - s * model_fn(xx, t.to(dev).expand(B)).double()) / a
    x = x.double()
    hist, t_hist = [x0_at(x, ts[0])], [ts[0]]
    for i in range(1, steps + 1):
        order = 1 if i == 1 or i == steps else 2                                        # warm-up; lower_order_final (steps < 10)
        lam_t, a_t, s_t = marg(ts[i])
        lam_0, _, s_0 = marg(t_hist[-1])
        h = lam_t - lam_0
        phi_1 = torch.expm1(torch.tensor(-h, dtype=torch.float64)).item()
        x_t = (s_t / s_0) * x - (a_t * phi_1) * hist[-1]
        if order == 2:
            r0 = (lam_0 - marg(t_hist[-2])[0]) / h
            x_t = x_t - 0.5 * (a_t * phi_1) * ((1. / r0) * (hist[-1] - hist[-2]))
        x = x_t
        if i < steps:
            hist, t_hist = (hist + [x0_at(x, ts[i])])[-2:], (t_hist + [ts[i]])[-2:]
    return x


@gpu
@pytest.mark.parametrize("model_type", ["noise", "v"])
def test_multistep_2_against_a_plain_torch_float64_loop(model_type):
    """the same comparison with NOTHING of the engine on the reference side: a torch float64 2M loop around
    WrappedModel.__call__, fed the recorded network outputs.  1e-5 of the scale."""
    ns = make_schedule("sd")
    rec = []
    x = x_T().to(DEV)
    got = D.DPM_Solver(wrap(conv_net(torch.float16, rec), ns, model_type, DEV), ns).sample(x, steps=6, order=2)
    want = torch_2m_float64(wrap(replay(rec, DEV), ns, model_type, DEV), ns, x, 6)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("cfg_rescale multistep-2 %s vs a torch float64 loop: %.3g of the scale" % (model_type, err))
    assert want.dtype is torch.float64 and err <= 1e-5


@gpu
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("method,order", RUNS)
def test_fp16_state_is_the_double_stage_by_stage(method, order, model_type, monkeypatch):
    ns = make_schedule("sd")
    algo = "dpmsolver" if (order == 2 and model_type == "noise") else "dpmsolver++"
    kw = dict(steps=6, order=order, method=method)
    rec = []
    x = x_T(torch.float16)
    mk = lambda net, dev: D.DPM_Solver(wrap(net, ns, model_type, dev), ns, algorithm_type=algo, state_dtype=torch.float16)
    got = mk(conv_net(torch.float16, rec), DEV).sample(x.to(DEV), **kw)
    assert got.dtype is torch.float16 and len(rec) == 6
    with monkeypatch.context() as m:
        RD.install_rescale_double(m, S, D)
        want = mk(replay(rec, "cpu"), "cpu").sample(x, **kw)
        wi = mk(replay(rec, "cpu"), "cpu").sample(x, return_intermediate=True, **kw)[1]
    assert torch.equal(got.cpu(), want)
    gi = mk(replay(rec, DEV), DEV).sample(x.to(DEV), return_intermediate=True, **kw)[1]      # the general loop, state by state
    assert len(gi) == len(wi) and all(torch.equal(a.cpu(), b) for a, b in zip(gi, wi))


@gpu
@pytest.mark.parametrize("sdt", [torch.float32, torch.float16])
def test_phi_0_is_bit_identical_to_the_wrapper_without_the_helper(sdt):
    ns = make_schedule("sd")
    x = x_T(sdt).to(DEV)
    kw = dict(steps=6, order=2)
    skw = dict(state_dtype=sdt) if sdt is torch.float16 else {}
    a = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV, phi=None), ns, **skw).sample(x, **kw)
    b = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV, phi=0.0), ns, **skw).sample(x, **kw)
    c = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV, phi=0.7), ns, **skw).sample(x, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)


@gpu
def test_capture_replay_equals_eager():
    ns = make_schedule("sd")
    x = x_T().to(DEV)
    dpm = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV), ns)
    eager = dpm.sample(x, steps=6, order=2)
    g = dpm.capture(x, steps=6, order=2)
    assert torch.equal(g(x), eager)
    x2 = x * 0.5 + 0.1
    assert torch.equal(g(x2), dpm.sample(x2, steps=6, order=2))


@gpu
def test_request_pool_without_slots_equals_two_sample_calls():
    ns = make_schedule("sd")
    dpm = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV), ns)
    xs = [x_T().to(DEV), (x_T() * 0.7 + 0.2).to(DEV)]
    kws = [dict(steps=6, order=2), dict(steps=5, order=3)]
    want = [dpm.sample(x, **kw) for x, kw in zip(xs, kws)]
    pool = dpm.request_pool()
    hs = [pool.submit(x, **kw) for x, kw in zip(xs, kws)]
    done = {}
    while pool:
        done.update(pool.step())
    assert all(torch.equal(done[h], w) for h, w in zip(hs, want))
    outs = dpm.sample_requests(xs, **kws[0])
    assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], dpm.sample(xs[1], **kws[0]))
