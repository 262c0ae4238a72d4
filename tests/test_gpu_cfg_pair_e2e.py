"""Guidance over two conditions end to end on the GPU: sample() through dpm_solver_amd.cfg_pair with a small convolutional
stand-in network at [3,4,16,16], 6 steps.  The network's outputs of the run under test are RECORDED and replayed to the
reference run, so both see the same tensors (a network re-evaluated on a state that differs in the last bit may round an output
element the other way, which is a property of the network, not of the solver):
  * against the engine's host code on the numpy double (tests/pair_double.py), bit for bit: sample(), return_intermediate state
    by state, sample_requests and capture; multistep order 2 and singlestep order 3, both algorithm types, fp16 and fp32 states;
    the same four paths under a [3B, 2C, H, W] network whose caller keeps C channels (a strided slice, made dense by the host);
  * an fp32 state with an fp16 network against a float64 statement of the same trajectory -- the conversions and the
    three-branch blend written out in torch float64 here (pair_noise_float64: nothing of the wrapper), inside a 2M loop in plain
    torch float64 for multistep order 2 and inside the engine's double-precision path for singlestep order 3 -- at the project's
    1e-5 of the scale;
  * WrappedModel.__call__ (the torch statement of the contract) against a one-stage DENOISE launch.
Run on an MI355X:  pytest -m gpu"""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import pair_double as PD
from apg_torch_ref import torch_2m_float64
from engine_cases import make_schedule

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (3, 4, 16, 16)
SCALE, SCALE2 = 7.5, 1.5                        # InstructPix2Pix's text and image scales (nested=True): s1 = 7.5, s2 = -6
RUNS = [("multistep", 2, "dpmsolver++"), ("multistep", 2, "dpmsolver"), ("singlestep", 3, "dpmsolver++"),
        ("singlestep", 3, "dpmsolver")]
RUN_IDS = ["%s-%d-%s" % r for r in RUNS]


def conv_net(dtype, record=None):
    """a 3x3 convolution over the channels plus terms in t and the condition -- the three thirds of a two-condition call differ
    in scale and offset; answers in `dtype`"""
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
    return D.cfg_pair(fn, 0.5 * c, SCALE2, nested=True) if on else fn     # (the inner condition between the two others)


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
    assert got.dtype is sdt and len(rec) == 6 and all(r.shape[0] == 3 * SHAPE[0] for r in rec)
    print("cfg_pair %s-%d %s %s %s: max |x_0| %.3g" % (method, order, algo, model_type, sdt, float(got.float().abs().max())))
    assert bool(torch.isfinite(got).all())
    with monkeypatch.context() as m:
        PD.install_pair_double(m, S, D)
        want = mk(replay(rec, "cpu"), "cpu").sample(x, **kw)
        wi = mk(replay(rec, "cpu"), "cpu").sample(x, return_intermediate=True, **kw)[1]
    assert torch.equal(got.cpu(), want)
    gi = mk(replay(rec, DEV), DEV).sample(x.to(DEV), return_intermediate=True, **kw)[1]      # the general loop, state by state
    assert len(gi) == len(wi) and all(torch.equal(a.cpu(), b) for a, b in zip(gi, wi))
    # two requests in flight: the first is the run above, the second another state on the same outputs
    outs = mk(replay([r for r in rec for _ in range(2)], DEV), DEV).sample_requests([x.to(DEV), x.to(DEV)], **kw)
    assert torch.equal(outs[0], got) and torch.equal(outs[1], got)
    # the second condition is not a no-op here: classifier-free guidance on the first two thirds gives another result
    two = [r[:2 * SHAPE[0]] for r in rec]
    plain = D.DPM_Solver(wrap(replay(two, DEV), ns, model_type, DEV, on=False), ns, algorithm_type=algo, **skw).sample(x.to(DEV), **kw)
    assert float((plain.float() - got.float()).abs().max() / got.float().abs().max()) > 1e-3


def pair_noise_float64(outs, ns, model_type):
    """model_fn(x, t[B]) -> noise in torch float64 from the recorded [3B, ...] outputs (unconditional, condition, condition2):
    InstructPix2Pix's formula on the converted outputs, every operation in double"""
    it = iter(outs)

    def fn(x, t):
        e_u, e_it, e_i = next(it).to(x.device).double().chunk(3)
        if model_type == "v":
            t64 = t.double().reshape(-1)
            al = ns.marginal_alpha(t64).reshape(-1, 1, 1, 1).double()
            sg = ns.marginal_std(t64).reshape(-1, 1, 1, 1).double()
            e_u, e_it, e_i = (al * o + sg * x.double() for o in (e_u, e_it, e_i))
        return e_u + SCALE2 * (e_i - e_u) + SCALE * (e_it - e_i)
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
        want = torch_2m_float64(pair_noise_float64(rec, ns, model_type), ns, x, 6)      # nothing of the engine
    else:
        want = D.DPM_Solver(pair_noise_float64(rec, ns, model_type), ns, algorithm_type=algo).sample(x.double(), **kw)
    assert want.dtype is torch.float64
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("cfg_pair %s-%d %s %s vs float64: %.3g of the scale" % (method, order, model_type, algo, err))
    assert err <= 1e-5


@gpu
def test_wrapper_call_is_the_one_stage_denoise_launch():
    """WrappedModel.__call__ -- the torch statement of the contract for callers other than DPM_Solver -- against
    noise_prediction_fn, one DENOISE launch of stage_pair_kernel: bit for bit on fp32 outputs (the same fp32 operations in the
    same order), noise and v; bit for bit on fp16 / bf16 outputs of a noise network too (widened exactly, then fp32); and at
    1e-5 of the scale on half outputs of a v network over an fp32 state."""
    ns = make_schedule("sd")
    x = x_T().to(DEV)
    t = torch.full((SHAPE[0],), 0.6, device=DEV)
    for mt in ("noise", "v"):
        fn = wrap(conv_net(torch.float32), ns, mt, DEV)
        a, b = fn(x, t), D.DPM_Solver(fn, ns, algorithm_type="dpmsolver").noise_prediction_fn(x, torch.tensor([0.6], device=DEV))
        assert a.dtype is torch.float32 and b.dtype is torch.float32
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        print("cfg_pair __call__ vs DENOISE launch, fp32 %s network: %.3g of the scale" % (mt, err))
        assert torch.equal(a, b) if mt == "noise" else err <= 1e-5
    off = wrap(conv_net(torch.float32), ns, "noise", DEV, on=False)
    fn = wrap(conv_net(torch.float32), ns, "noise", DEV)
    assert float((off(x, t) - fn(x, t)).abs().max() / fn(x, t).abs().max()) > 1e-3       # the second condition is not a no-op
    for hd in (torch.float16, torch.bfloat16):
        fn = wrap(conv_net(hd), ns, "v", DEV)
        a, b = fn(x, t), D.DPM_Solver(fn, ns).noise_prediction_fn(x, torch.tensor([0.6], device=DEV))
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        print("cfg_pair __call__ vs DENOISE launch, v network in %s: %.3g of the scale" % (hd, err))
        assert a.dtype is torch.float32 and b.dtype is torch.float32 and err <= 1e-5


class Recording:
    """`net` with its outputs appended to `rec` while `on` (a capture's warm-up runs and the capture itself record nothing)"""

    def __init__(self, net):
        self.net, self.rec, self.on = net, [], False

    def __call__(self, x, t, c):
        out = self.net(x, t, c)
        if self.on:
            self.rec.append(out.clone())
        return out

    def run(self, fn):
        self.rec, self.on = [], True
        try:
            return fn(), self.rec
        finally:
            self.on = False


def wide(net):
    """a learned-variance network: it answers [3B, 2C, H, W] and its caller keeps the first C channels -- `out[:, :C]`, a channel
    slice whose samples are dense but lie a wide output's stride apart, which the two-branch kernels read in place (eps_stride)"""
    def f(x, t, c):
        y = net(x, t, c)
        return torch.cat([y, 0.5 * y - 1.0], dim=1)[:, :y.shape[1]]
    return f


@gpu
@pytest.mark.parametrize("sdt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_capture_replay_equals_eager_and_the_double(sdt, monkeypatch):
    """a captured graph's replay against the eager run, whose recorded outputs give the double's result: all three bit for bit"""
    ns = make_schedule("sd")
    kw = dict(steps=6, order=2)
    skw = dict(state_dtype=sdt) if sdt is torch.float16 else {}
    x = x_T(sdt)
    net = Recording(pointwise_net)
    dpm = D.DPM_Solver(wrap(net, ns, "v", DEV), ns, **skw)
    eager, rec = net.run(lambda: dpm.sample(x.to(DEV), **kw))
    assert eager.dtype is sdt and len(rec) == 6 and all(r.shape[0] == 3 * SHAPE[0] for r in rec)
    with monkeypatch.context() as m:
        PD.install_pair_double(m, S, D)
        want = D.DPM_Solver(wrap(replay(rec, "cpu"), ns, "v", "cpu"), ns, **skw).sample(x, **kw)
    assert torch.equal(eager.cpu(), want)
    g = dpm.capture(x.to(DEV), **kw)
    assert torch.equal(g(x.to(DEV)), eager)
    x2 = (x.float() * 0.5 + 0.1).to(sdt).to(DEV)
    eager2, rec2 = net.run(lambda: dpm.sample(x2, **kw))
    with monkeypatch.context() as m:
        PD.install_pair_double(m, S, D)
        want2 = D.DPM_Solver(wrap(replay(rec2, "cpu"), ns, "v", "cpu"), ns, **skw).sample(x2.cpu(), **kw)
    assert torch.equal(g(x2), eager2) and torch.equal(eager2.cpu(), want2)
    off = D.DPM_Solver(wrap(pointwise_net, ns, "v", DEV, on=False), ns, **skw).sample(x.to(DEV), **kw)
    assert not torch.equal(eager, off)


@gpu
@pytest.mark.parametrize("sdt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_a_channel_slice_of_a_wider_output_is_made_dense_on_every_path(sdt, monkeypatch):
    """A [3B, 2C, H, W] network sliced to C channels: sample(), return_intermediate, sample_requests and capture() -- the
    prebuilt launch records, the general loop, the multi-request call and a graph -- against the double on the recorded
    (dense) outputs, bit for bit.  stage_pair_kernel takes no eps_stride slice, so each path binds three dense copies."""
    ns = make_schedule("sd")
    kw = dict(steps=6, order=2)
    skw = dict(state_dtype=sdt) if sdt is torch.float16 else {}
    x = x_T(sdt)
    rec = []
    mk = lambda net, dev: D.DPM_Solver(wrap(net, ns, "noise", dev), ns, **skw)
    probe = wide(conv_net(sdt))(x.to(DEV).repeat(3, 1, 1, 1), torch.zeros(9, device=DEV), torch.zeros(9, device=DEV))
    assert probe.shape[1:] == SHAPE[1:] and not probe.is_contiguous() and probe.stride(0) == 2 * probe[0].numel()
    got = mk(wide(conv_net(sdt, rec)), DEV).sample(x.to(DEV), **kw)
    assert got.dtype is sdt and len(rec) == 6
    with monkeypatch.context() as m:
        PD.install_pair_double(m, S, D)
        want = mk(replay(rec, "cpu"), "cpu").sample(x, **kw)
        wi = mk(replay(rec, "cpu"), "cpu").sample(x, return_intermediate=True, **kw)[1]
    assert torch.equal(got.cpu(), want)
    gi = mk(wide(replay(rec, DEV)), DEV).sample(x.to(DEV), return_intermediate=True, **kw)[1]
    assert len(gi) == len(wi) and all(torch.equal(a.cpu(), b) for a, b in zip(gi, wi))
    outs = mk(wide(replay([r for r in rec for _ in range(2)], DEV)), DEV).sample_requests([x.to(DEV), x.to(DEV)], **kw)
    assert torch.equal(outs[0], got) and torch.equal(outs[1], got)
    # capture: a network that is a function of its inputs alone (a replayed list cannot sit in a graph)
    dpm = mk(wide(pointwise_net), DEV)
    dense = mk(pointwise_net, DEV).sample(x.to(DEV), **kw)                   # the same values from a dense network
    assert torch.equal(dpm.sample(x.to(DEV), **kw), dense)
    assert torch.equal(dpm.capture(x.to(DEV), **kw)(x.to(DEV)), dense)


@gpu
def test_sample_requests_equals_the_sample_calls_and_a_double_state_runs():
    ns = make_schedule("sd")
    dpm = D.DPM_Solver(wrap(pointwise_net, ns, "noise", DEV), ns)
    xs = [x_T().to(DEV), (x_T() * 0.7 + 0.2).to(DEV)]
    kw = dict(steps=6, order=2, denoise_to_zero=True)
    want = [dpm.sample(x, **kw) for x in xs]
    outs = dpm.sample_requests(xs, **kw)
    assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])
    # a double state blends the three outputs in torch: the fp32 run's result within fp32 rounding
    d = dpm.sample(xs[0].double(), **kw)
    assert d.dtype is torch.float64 and float((d - want[0].double()).abs().max() / d.abs().max()) <= 1e-5
