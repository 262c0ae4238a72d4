"""Every message of dpm_solver_amd/slab.py that the public API can reach without a GPU, whole: the exception's type and its
full text compared with == against a literal (the other slab tests match fragments).  On a host tensor: `_refuse`,
`_guidance`, `_check_state` and the blend= / seed= checks of `submit`.  With tests/table_double.py installed, what sits behind
the device requirement: `_conditions`, the checks of `_enqueue` and `_check_state` on the pool's own shape, an `intermediates`
entry of the wrong shape, and `_bind` on the network's output.  And the order where two refusals compete.

Not reached here: "ticks are not captured into graphs" (needs a capturing stream), "a plan with %d cached model values" (no
order the planner accepts caches more than three) and "the request has no unconditional_condition" (a wrapper without one is
not effectively classifier-free, and asks for none)."""
import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import table_blend_double as TBD
import table_double as TD
from engine_cases import make_schedule
from test_slab_pool_host import _net, _plain
from test_slab_pool_host import _solver as _cfg
from test_slab_rescale_host import _solver as _rescale

NS = make_schedule("sd")
TAIL = "; use request_pool() without slots"


def _raises(exc, text, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc and str(e.value) == text


def test_refuse_messages():
    x = torch.randn(2, 4, 8, 8)
    pool = _plain().request_pool(slots=8)
    for method in ("singlestep", "adaptive"):
        _raises(NotImplementedError, "slab pool: method=%r -- a singlestep or adaptive update evaluates the network on an "
                "intermediate state, and a slab row's evaluation state is its state" % method + TAIL,
                pool.submit, x, steps=6, method=method)
    _raises(NotImplementedError, "slab pool: sde=True -- SDE stages have no table kernel" + TAIL, pool.submit, x, steps=6, sde=True)
    _raises(NotImplementedError, "slab pool: correcting_x0_fn='dynamic_thresholding' -- thresholded stages have no table kernel"
            + TAIL, _plain(correcting_x0_fn="dynamic_thresholding").request_pool(slots=8).submit, x, steps=6)
    clf = D.DPM_Solver(D.model_wrapper(_net, NS, guidance_type="classifier", condition=torch.ones(1),
                                       classifier_fn=lambda x, t, c: x.sum()), NS, algorithm_type="dpmsolver++")
    _raises(NotImplementedError, "slab pool: classifier guidance -- the classifier's gradient is a second network call per "
            "request" + TAIL, clf.request_pool(slots=8).submit, x, steps=6)
    for kw in (dict(correcting_x0_fn=lambda x0, t: x0), dict(correcting_xt_fn=lambda xt, t, step: xt)):
        _raises(NotImplementedError, "slab pool: a correcting_x0_fn / correcting_xt_fn runs Python between stages; sample with "
                "sample()", _plain(**kw).request_pool(slots=8).submit, x, steps=6)
    for submit in (pool.submit, pool.submit_unipc):
        _raises(NotImplementedError, "slab pool: return_intermediate is not supported; sample it with sample()",
                submit, x, steps=6, return_intermediate=True)
    _raises(ValueError, "slab pool: `seed` / `generator` belong to an SDE request (sde=True)", pool.submit, x, steps=6, seed=3)
    _raises(ValueError, "slab pool: `seed` / `generator` belong to an SDE request (sde=True)",
            pool.submit, x, steps=6, generator=torch.Generator())


def test_guidance_messages():
    x = torch.randn(2, 4, 8, 8)
    pool = _rescale(torch.float32, 3.0, 0.7).request_pool(slots=8, rescale=True)
    plain = _rescale(torch.float32, 3.0, 0.0).request_pool(slots=8)
    uncond = _rescale(torch.float32, cfg=False).request_pool(slots=8)
    belong = ("slab pool: guidance_scale / guidance_rescale belong to a classifier-free wrapper (with an unconditional "
              "condition and a guidance scale other than 1)")
    _raises(ValueError, belong, uncond.submit, x, steps=6, guidance_scale=2.0)
    _raises(ValueError, belong, uncond.submit, x, steps=6, guidance_rescale=0.5)
    _raises(ValueError, belong, uncond.submit_unipc, x, steps=6, guidance_scale=2.0)
    _raises(ValueError, "slab pool: guidance_scale must be a real number, got '3'", pool.submit, x, steps=6, guidance_scale="3")
    _raises(ValueError, "slab pool: guidance_scale must be a real number, got True", pool.submit, x, steps=6, guidance_scale=True)
    _raises(ValueError, "slab pool: guidance_scale must be a real number, got nan", pool.submit, x, steps=6,
            guidance_scale=float("nan"))
    _raises(ValueError, "slab pool: guidance_rescale must be a real number, got '0.5'",
            pool.submit, x, steps=6, guidance_rescale="0.5")
    _raises(ValueError, "slab pool: guidance_rescale must be in [0, 1], got 1.5", pool.submit, x, steps=6, guidance_rescale=1.5)
    _raises(ValueError, "slab pool: guidance_rescale must be in [0, 1], got -0.1", pool.submit, x, steps=6, guidance_rescale=-0.1)
    scale1 = ("slab pool: guidance_scale=1.0 -- a wrapper of scale 1 evaluates the conditional branch alone, without a blend, "
              "which a row of a classifier-free slab cannot reproduce")
    _raises(NotImplementedError, scale1, pool.submit, x, steps=6, guidance_scale=1.0)
    _raises(NotImplementedError, scale1, plain.submit_unipc, x, steps=6, guidance_scale=1)
    outside = ("slab pool: guidance_rescale= -- rescale stages take the table in a pool built with request_pool(slots=..., "
               "rescale=True) only")
    _raises(NotImplementedError, outside, plain.submit, x, steps=6, guidance_rescale=0.5)
    # two refusals compete: scale 1 comes before the phi of a pool without rescale=True
    _raises(NotImplementedError, scale1, plain.submit, x, steps=6, guidance_scale=1.0, guidance_rescale=0.5)


def test_check_state_messages():
    x = torch.randn(2, 4, 8, 8)
    _raises(NotImplementedError, "slab pool: double-precision states (the table kernels take 2- and 4-byte states)",
            _plain().request_pool(slots=8).submit, x.double(), steps=6)
    lin = D.NoiseScheduleVP("linear")
    half = D.DPM_Solver(D.model_wrapper(_net, lin), lin, algorithm_type="dpmsolver++")
    _raises(NotImplementedError, "slab pool: a half-precision slab needs a solver built with an explicit state_dtype -- the "
            "reference's type promotion would depend on the first network output", half.request_pool(slots=8).submit, x.half(), steps=6)
    groups = " elements -- %s whole 8-element groups of 16-byte aligned buffers" + TAIL
    sde = "slab pool: sde=True with a sample of %d" + groups % "a row of the table noise kernel is"
    rsc = "slab pool: rescale=True with a sample of %d" + groups % "a rescale row of the table is"
    thr = ("slab pool: thresholding=True with a sample of %d"
           + groups % "a thresholded row of the table is at most 12288 elements (one workgroup's LDS),")
    small, odd, big = torch.randn(2, 1, 2, 2), torch.randn(2, 3, 2, 2), torch.randn(1, 3, 64, 72)
    thresholding = _plain(correcting_x0_fn="dynamic_thresholding")
    for xx, per in ((small, 4), (odd, 12)):
        _raises(NotImplementedError, sde % per, _plain().request_pool(slots=8, sde=True).submit, xx, steps=6)
        _raises(NotImplementedError, thr % per, thresholding.request_pool(slots=8, thresholding=True).submit, xx, steps=6)
        _raises(NotImplementedError, rsc % per, _rescale(torch.float32, 3.0, 0.7).request_pool(slots=8, rescale=True).submit,
                xx, steps=6)
    _raises(NotImplementedError, thr % 13824, thresholding.request_pool(slots=8, thresholding=True).submit, big, steps=6)
    # two refusals compete: the SDE check of a pool built with both comes first
    _raises(NotImplementedError, sde % 12, thresholding.request_pool(slots=8, sde=True, thresholding=True).submit, odd, steps=6)


def test_blend_messages():
    x = torch.randn(2, 4, 8, 8)
    mask = torch.ones(8, 8)
    mb = D.MaskBlend(NS, mask, x0=torch.randn(2, 4, 8, 8), noise=torch.randn(2, 4, 8, 8))
    dpm = _plain()
    without = "slab pool: blend= -- mask-blend stages take the table in a pool built with request_pool(slots=..., inpaint=True) only"
    _raises(NotImplementedError, without, dpm.request_pool(slots=8).submit, x, steps=6, blend=mb)
    _raises(NotImplementedError, without, dpm.request_pool(slots=8, sde=True).submit, x, steps=6, blend=mb)
    pool = dpm.request_pool(slots=8, inpaint=True)
    _raises(NotImplementedError, "slab pool: blend= takes a dpm_solver_amd.MaskBlend (any other correcting_xt_fn runs Python "
            "between stages; sample with sample())", pool.submit, x, steps=6, blend=lambda x, t, step: x)
    _raises(NotImplementedError, "slab pool: blend= with sde=True -- the table has no blend behind the noise epilogue; sample it "
            "with sample_sde()", dpm.request_pool(slots=8, inpaint=True, sde=True).submit, x, steps=6, order=2, sde=True, seed=1,
            blend=mb)
    _raises(NotImplementedError, "slab pool: MaskBlend(x0=..., noise=None) draws torch.randn per call, which a pool cannot "
            "reproduce; pass noise= (the fixed-noise re-noising of the known image)",
            pool.submit, x, steps=6, blend=D.MaskBlend(NS, mask, x0=torch.randn(2, 4, 8, 8)))


# ---- behind the device requirement: tests/table_double.py stands in for the device
def test_condition_messages(monkeypatch):
    TD.install_table_double(monkeypatch, S, D)
    x = torch.randn(2, 4, 8, 8)
    belong = "slab pool: `condition` / `unconditional_condition` belong to a classifier-free wrapper"
    _raises(ValueError, belong, _plain().request_pool(slots=4).submit, x, steps=5, condition=torch.ones(2, 1))
    _raises(ValueError, belong, _plain().request_pool(slots=4).submit_unipc, x, steps=5, unconditional_condition=torch.ones(2, 1))
    pool = _cfg(True, torch.float32).request_pool(slots=4)
    _raises(ValueError, "slab pool: condition must be a tensor of leading dimension 2 or 1",
            pool.submit, x, steps=5, condition=torch.ones(3, 1))
    _raises(ValueError, "slab pool: unconditional_condition must be a tensor of leading dimension 2 or 1",
            pool.submit, x, steps=5, unconditional_condition=[0.0])
    differ = "slab pool: condition and unconditional_condition differ in shape or dtype"
    _raises(ValueError, differ, pool.submit, x, steps=5, condition=torch.ones(2, 3))
    _raises(ValueError, differ, pool.submit, x, steps=5, unconditional_condition=torch.zeros(1, 1, dtype=torch.float16))
    assert pool._like is None                                                   # (nothing was allocated on the way)
    pool.submit(x, steps=5)
    _raises(ValueError, "slab pool: a condition of shape (3,), dtype torch.float32 does not match the pool's (1,), torch.float32",
            pool.submit, x, steps=5, condition=torch.ones(2, 3), unconditional_condition=torch.zeros(1, 3))
    fn = D.model_wrapper(_net, NS, guidance_type="classifier-free", guidance_scale=3.0, condition=None,
                         unconditional_condition=torch.zeros(1, 1))
    none = D.DPM_Solver(fn, NS, algorithm_type="dpmsolver++").request_pool(slots=4)
    _raises(ValueError, "slab pool: the request has no condition and the wrapper has none", none.submit, x, steps=5)


def test_shape_messages(monkeypatch):
    TD.install_table_double(monkeypatch, S, D)
    pool = _plain().request_pool(slots=4)
    _raises(ValueError, "slab pool: x must be a tensor [b, *sample_shape] with at least one element",
            pool.submit, torch.randn(0, 4, 8, 8), steps=5)
    _raises(ValueError, "slab pool: a request of 5 samples does not fit 4 slots", pool.submit, torch.randn(5, 4, 8, 8), steps=5)
    pool.submit(torch.randn(2, 4, 8, 8), steps=5)
    _raises(ValueError, "slab pool: x of sample shape (4, 8, 9), dtype torch.float32 on cpu does not match the pool's (4, 8, 8), "
            "torch.float32 on cpu", pool.submit, torch.randn(1, 4, 8, 9), steps=5)
    _raises(ValueError, "slab pool: a request of 5 samples does not fit 4 slots", pool.submit, torch.randn(5, 4, 8, 8), steps=5)


def test_intermediates_message(monkeypatch):
    TBD.install_table_blend_double(monkeypatch, S, D)
    pool = _plain().request_pool(slots=4, inpaint=True)
    mb = D.MaskBlend(NS, torch.ones(8, 8), intermediates=[torch.randn(1, 4, 8, 8)] * 8)
    _raises(ValueError, "slab pool: intermediates[1] of shape (1, 4, 8, 8) for a state of (2, 4, 8, 8)",
            pool.submit, torch.randn(2, 4, 8, 8), steps=5, blend=mb)


def test_bind_messages(monkeypatch):
    TD.install_table_double(monkeypatch, S, D)
    x = torch.randn(2, 4, 8, 8)
    narrow = D.DPM_Solver(D.model_wrapper(lambda x, t: x[:, :2], NS), NS, algorithm_type="dpmsolver++").request_pool(slots=4)
    narrow.submit(x, steps=5)
    _raises(NotImplementedError, "slab pool: a network output of shape (4, 2, 8, 8) for an input of (4, 4, 8, 8) (channel slices "
            "of a wider output are not bound per row)", narrow.step)
    double = D.DPM_Solver(D.model_wrapper(lambda x, t: x.double(), NS), NS, algorithm_type="dpmsolver++").request_pool(slots=4)
    double.submit(x, steps=5)
    _raises(NotImplementedError, "slab pool: a double network output promotes the state to double", double.step)
