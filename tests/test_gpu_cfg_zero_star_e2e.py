"""CFG-Zero* end to end on the GPU: sample() through dpm_solver_amd.cfg_zero_star with a small convolutional stand-in network
at [3,4,16,16], 6 steps.  The network's outputs of the run under test are RECORDED and replayed to the reference run, so both
see the same tensors (a network re-evaluated on a state that differs in the last bit may round an output element the other
way, which is a property of the network, not of the solver):
  * against the engine's host code on the numpy double (tests/zstar_double.py), bit for bit: sample(), return_intermediate
    state by state, sample_requests and capture; multistep order 2 and singlestep order 3, both algorithm types, fp16 and
    fp32 states;
  * an fp32 state with an fp16 network against a float64 statement of the same trajectory -- the projection, the blend and
    the conversion written out in torch float64 here (zstar_noise_float64: nothing of the wrapper), inside a 2M loop in plain
    torch float64 for multistep order 2 and inside the engine's double-precision path for singlestep order 3 -- at the
    project's 1e-5 of the scale; measured on an MI355X: profiles/r27_cfg_zero_star.md;
  * WrappedModel.__call__ (the torch statement of the contract) against a one-stage DENOISE launch.
Run on an MI355X:  pytest -m gpu"""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import zstar_double as ZD
from apg_torch_ref import torch_2m_float64
from engine_cases import make_schedule

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (3, 4, 16, 16)
SCALE = 7.5
RUNS = [("multistep", 2, "dpmsolver++"), ("multistep", 2, "dpmsolver"), ("singlestep", 3, "dpmsolver++"),
        ("singlestep", 3, "dpmsolver")]
RUN_IDS = ["%s-%d-%s" % r for r in RUNS]


def conv_net(dtype, record=None):
    """a 3x3 convolution over the channels plus terms in t and the condition -- the two halves of a classifier-free call
    differ in scale and offset; answers in `dtype`"""
    w = (torch.randn(4, 4, 3, 3, generator=torch.Generator().manual_seed(3)) * 0.15)

    def net(x, t, c):
        cc = c.reshape(-1, 1, 1, 1).float()
        y = torch.nn.functional.conv2d(x.float(), w.to(x.device), padding=1) + 0.3 * torch.tanh(x.float())
        y = y * (0.6 + 0.2 * cc) + 0.05 * cc + 0.0002 * t.reshape(-1, 1, 1, 1).float()
        out = y.to(dtype)
        if record is not None:
            record.append(out)
        return out
    return net


def pointwise_net(x, t, c):
    cc = c.reshape(-1, 1, 1, 1)
    return (torch.tanh(x * 0.7) * (0.5 + 0.1 * cc) + 0.05 * x + 0.1 * cc).to(x.dtype)


def wrap(net, ns, model_type, device, on=True):
    c = torch.tensor([1.0, 2.0, 3.0], device=device)
    fn = D.model_wrapper(net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=SCALE, condition=c,
                         unconditional_condition=c * 0)
    return D.cfg_zero_star(fn) if on else fn


def replay(outs, device, dtype=None):
    it = iter(outs)

    def net(x, t, c):
        o = next(it).to(device)
        return o if dtype is None else o.to(dtype)
    return net


def x_T(dtype=torch.float32):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(11)).to(dtype)


@gpu
@pytest.mark.parametrize("sdt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("method,order,algo", RUNS, ids=RUN_IDS)
def test_sample_is_the_double_stage_by_stage(method, order, algo, model_type, sdt, monkeypatch):
    ns = make_schedule("sd")
    kw = dict(steps=6, order=order, method=method)
    rec = []
    x = x_T(sdt)
    skw = dict(state_dtype=sdt) if sdt is torch.float16 else {}
    mk = lambda net, dev: D.DPM_Solver(wrap(net, ns, model_type, dev), ns, algorithm_type=algo, **skw)
    got = mk(conv_net(sdt, rec), DEV).sample(x.to(DEV), **kw)
    assert got.dtype is sdt and len(rec) == 6
    with monkeypatch.context() as m:
        ZD.install_zstar_double(m, S, D)                                      # (asserts every stage's inputs decidable)
        want = mk(replay(rec, "cpu"), "cpu").sample(x, **kw)
        wi = mk(replay(rec, "cpu"), "cpu").sample(x, return_intermediate=True, **kw)[1]
    assert torch.equal(got.cpu(), want)
    gi = mk(replay(rec, DEV), DEV).sample(x.to(DEV), return_intermediate=True, **kw)[1]      # the general loop, state by state
    assert len(gi) == len(wi) and all(torch.equal(a.cpu(), b) for a, b in zip(gi, wi))
    # two requests in flight: the first is the run above, the second another state on the same outputs
    outs = mk(replay([r for r in rec for _ in range(2)], DEV), DEV).sample_requests([x.to(DEV), x.to(DEV)], **kw)
    assert torch.equal(outs[0], got) and torch.equal(outs[1], got)
    # the projection is not a no-op here: without it the same outputs give another result
    plain = D.DPM_Solver(wrap(replay(rec, DEV), ns, model_type, DEV, on=False), ns, algorithm_type=algo, **skw).sample(x.to(DEV), **kw)
    assert float((plain.float() - got.float()).abs().max() / got.float().abs().max()) > 1e-3


def zstar_noise_float64(outs, ns, model_type):
    """model_fn(x, t[B]) -> noise in torch float64 from the recorded [2B, ...] outputs (unconditional half first): the
    contract's formulas, every operation in double"""
    it = iter(outs)

    def fn(x, t):
        e1, e0 = next(it).to(x.device).double().chunk(2)
        axes = list(range(1, x.dim()))
        a = (e0 * e1).sum(dim=axes, keepdim=True) / ((e1 * e1).sum(dim=axes, keepdim=True) + 1e-8)
        u = a * e1
        g = u + SCALE * (e0 - u)
        if model_type == "noise":
            return g
        t64 = t.double().reshape(-1)
        al = ns.marginal_alpha(t64).reshape(-1, 1, 1, 1).double()
        sg = ns.marginal_std(t64).reshape(-1, 1, 1, 1).double()
        return al * g + sg * x.double()                                       # "v"
    return fn


@gpu
@pytest.mark.parametrize("model_type", ["noise", "v"])
@pytest.mark.parametrize("method,order,algo", RUNS, ids=RUN_IDS)
def test_fp32_state_fp16_network_against_a_float64_statement(method, order, algo, model_type):
    ns = make_schedule("sd")
    kw = dict(steps=6, order=order, method=method)
    rec = []
    x = x_T().to(DEV)
    got = D.DPM_Solver(wrap(conv_net(torch.float16, rec), ns, model_type, DEV), ns, algorithm_type=algo).sample(x, **kw)
    assert got.dtype is torch.float32 and len(rec) == 6
    if method == "multistep" and algo == "dpmsolver++":
        want = torch_2m_float64(zstar_noise_float64(rec, ns, model_type), ns, x, 6)     # nothing of the engine
    else:
        want = D.DPM_Solver(zstar_noise_float64(rec, ns, model_type), ns, algorithm_type=algo).sample(x.double(), **kw)
    assert want.dtype is torch.float64
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("cfg_zero_star %s-%d %s %s vs float64: %.3g of the scale" % (method, order, model_type, algo, err))
    assert err <= 1e-5


@gpu
def test_wrapper_call_is_the_one_stage_denoise_launch():
    """WrappedModel.__call__ -- the torch statement of the contract for callers other than DPM_Solver -- against
    noise_prediction_fn, one DENOISE launch of stage_zstar_kernel: bit for bit on an fp32 noise network (the same fp32
    operations in the same order, a from float64 sums), and at 1e-5 of the scale on fp16 / bf16 outputs of a v network over
    an fp32 state (the schedule's scalars meet the output in a different order of fp32 operations)."""
    ns = make_schedule("sd")
    x = x_T().to(DEV)
    t = torch.full((SHAPE[0],), 0.6, device=DEV)
    fn = wrap(conv_net(torch.float32), ns, "noise", DEV)
    dpm = D.DPM_Solver(fn, ns)
    a, b = fn(x, t), dpm.noise_prediction_fn(x, torch.tensor([0.6], device=DEV))
    assert a.dtype is torch.float32 and torch.equal(a, b)
    off = wrap(conv_net(torch.float32), ns, "noise", DEV, on=False)
    assert float((off(x, t) - a).abs().max() / a.abs().max()) > 1e-3          # the projection is not a no-op here
    for hd in (torch.float16, torch.bfloat16):
        fn = wrap(conv_net(hd), ns, "v", DEV)
        a, b = fn(x, t), D.DPM_Solver(fn, ns).noise_prediction_fn(x, torch.tensor([0.6], device=DEV))
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        print("cfg_zero_star __call__ vs DENOISE launch, v network in %s: %.3g of the scale" % (hd, err))
        assert a.dtype is torch.float32 and b.dtype is torch.float32 and err <= 1e-5


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
    assert not torch.equal(eager, D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV, on=False), ns).sample(x, steps=6, order=2))


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
