"""Adaptive projected guidance end to end on the GPU: sample() through dpm_solver_amd.cfg_apg (eta 0.5, a norm threshold that
caps, momentum -0.5) with a small convolutional stand-in network at [2,4,16,16], 6 steps.  The network's outputs of the run
under test are RECORDED and replayed to the reference run, so both see the same half-precision tensors (a network re-evaluated on
a state that differs in the last bit may round an output element the other way, which is a property of the network, not of the
solver):
  * an fp32 state with an fp16 network against the guidance written out in plain torch float64 (tests/apg_torch_ref.py:
    ApgModel64, which carries its own running average and shares nothing with the project's wrapper), at 1e-5 of the scale
    (DESIGN section 7): for multistep order 2 inside a 2M loop written out in torch float64 as well (no planner, no kernel of the
    project), for every method inside the engine's double-precision path on x.double() (the planner's stage order is the order of
    the network evaluations, which is what the running average follows);
  * an fp16 state against the engine's host code on the numpy double (tests/apg_double.py), stage by stage, bit for bit;
  * a RequestPool of three staggered requests with a momentum against sample() on each alone, bit for bit.
Run on an MI355X:  pytest -m gpu"""
import pytest
import torch

import apg_double as AD
import dpm_solver_amd as D
import dpm_solver_amd.solver as S
from apg_torch_ref import ApgModel64, torch_2m_float64
from engine_cases import make_schedule

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (2, 4, 16, 16)
RUNS = [("multistep", 2), ("multistep", 3), ("singlestep", 3)]
SCALE = 7.5
APG = (0.5, 4.0, -0.5)       # eta, norm threshold (the direction of a [4,16,16] sample here has a norm of tens: it caps), momentum


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


def wrap(net, ns, model_type, device, apg=APG):
    c = torch.tensor([1.0, 2.0], device=device)
    fn = D.model_wrapper(net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=SCALE, condition=c,
                         unconditional_condition=c * 0)
    return fn if apg is None else D.cfg_apg(fn, *apg)


def replay(outs, device, dtype=None):
    it = iter(outs)

    def net(x, t, c):
        o = next(it).to(device)
        return o if dtype is None else o.to(dtype)
    return net


def replay_pair(outs, device):
    """the recorded [2B, ...] outputs (unconditional half first, as the wrapper batches them) as raw(x, t) -> (cond, uncond)"""
    it = iter(outs)

    def raw(x, t):
        e1, e0 = next(it).to(device).chunk(2)
        return e0, e1
    return raw


def x_T(dtype=torch.float32):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(11)).to(dtype)


@gpu
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("method,order", RUNS)
def test_fp32_state_fp16_network_against_plain_torch_float64(method, order, model_type):
    ns = make_schedule("sd")
    kw = dict(steps=6, order=order, method=method)
    rec = []
    x = x_T().to(DEV)
    got = D.DPM_Solver(wrap(conv_net(torch.float16, rec), ns, model_type, DEV), ns).sample(x, **kw)
    assert got.dtype is torch.float32 and len(rec) == 6
    ref_fn = ApgModel64(replay_pair(rec, DEV), ns, model_type, SCALE, *APG)
    want = D.DPM_Solver(lambda xx, t: ref_fn(xx, t), ns).sample(x.double(), **kw)
    assert want.dtype is torch.float64
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("cfg_apg %s-%d %s vs torch float64 guidance: %.3g of the scale" % (method, order, model_type, err))
    assert err <= 1e-5
    if (method, order) == ("multistep", 2):        # ... and with NOTHING of the engine on the reference side
        want2 = torch_2m_float64(ApgModel64(replay_pair(rec, DEV), ns, model_type, SCALE, *APG), ns, x, 6)
        err2 = float((got.double() - want2).abs().max() / want2.abs().max())
        print("cfg_apg multistep-2 %s vs a torch float64 loop: %.3g of the scale" % (model_type, err2))
        assert want2.dtype is torch.float64 and err2 <= 1e-5
    # the guidance is not a no-op here, and neither is its momentum: without either the same outputs give another result
    for other in (None, (APG[0], APG[1], 0.0)):
        plain = D.DPM_Solver(wrap(replay(rec, DEV), ns, model_type, DEV, apg=other), ns).sample(x, **kw)
        assert float((plain - got).abs().max() / want.abs().max()) > 1e-3


@gpu
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("method,order", RUNS)
def test_fp16_state_is_the_double_stage_by_stage(method, order, model_type, monkeypatch):
    ns = make_schedule("sd")
    kw = dict(steps=6, order=order, method=method)
    rec = []
    x = x_T(torch.float16)
    mk = lambda net, dev: D.DPM_Solver(wrap(net, ns, model_type, dev), ns, state_dtype=torch.float16)
    got = mk(conv_net(torch.float16, rec), DEV).sample(x.to(DEV), **kw)
    assert got.dtype is torch.float16 and len(rec) == 6
    with monkeypatch.context() as m:
        AD.install_apg_double(m, S, D)
        want = mk(replay(rec, "cpu"), "cpu").sample(x, **kw)
        wi = mk(replay(rec, "cpu"), "cpu").sample(x, return_intermediate=True, **kw)[1]
    assert torch.equal(got.cpu(), want)
    gi = mk(replay(rec, DEV), DEV).sample(x.to(DEV), return_intermediate=True, **kw)[1]      # the general loop, state by state
    assert len(gi) == len(wi) and all(torch.equal(a.cpu(), b) for a, b in zip(gi, wi))


@gpu
def test_request_pool_of_three_staggered_requests_equals_sample_on_each():
    ns = make_schedule("sd")
    dpm = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV), ns)
    xs = [x_T().to(DEV), (x_T() * 0.7 + 0.2).to(DEV), (x_T() * 1.1 - 0.1).to(DEV)]
    kws = [dict(steps=6, order=2), dict(steps=5, order=3), dict(steps=4, order=2, denoise_to_zero=True)]
    want = [dpm.sample(x, **kw) for x, kw in zip(xs, kws)]
    pool = dpm.request_pool()
    hs, done = [], {}
    for x, kw in zip(xs, kws):                    # a request joins every second tick: three positions in flight at once
        hs.append(pool.submit(x, **kw))
        done.update(pool.step())
        done.update(pool.step())
    while pool:
        done.update(pool.step())
    assert all(torch.equal(done[h], w) for h, w in zip(hs, want))
    # a request that reuses a finished one's records starts from a zero average
    h = pool.submit(xs[0], **kws[0])
    while pool:
        done.update(pool.step())
    assert torch.equal(done[h], want[0])
    outs = dpm.sample_requests(xs[:2], **kws[0])
    assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], dpm.sample(xs[1], **kws[0]))


@gpu
def test_the_identity_is_bit_identical_to_the_wrapper_without_the_helper():
    ns = make_schedule("sd")
    x = x_T().to(DEV)
    kw = dict(steps=6, order=2)
    a = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV, apg=None), ns).sample(x, **kw)
    b = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV, apg=(1.0, 0.0, 0.0)), ns).sample(x, **kw)
    c = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV), ns).sample(x, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)


@gpu
def test_capture_replay_equals_eager_without_a_momentum():
    ns = make_schedule("sd")
    x = x_T().to(DEV)
    dpm = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV, apg=(APG[0], APG[1], 0.0)), ns)
    eager = dpm.sample(x, steps=6, order=2)
    g = dpm.capture(x, steps=6, order=2)
    assert torch.equal(g(x), eager)
    x2 = x * 0.5 + 0.1
    assert torch.equal(g(x2), dpm.sample(x2, steps=6, order=2))
    with pytest.raises(NotImplementedError, match="capture with a momentum"):
        D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV), ns).capture(x, steps=6, order=2)
