"""GPU tests of the fused multi-request launch's store policy for 2-byte states (MultiShape: new state written through, model
value by a non-temporal store): the fused trajectories must end bit-identical to the same requests advanced one launch per
request (dpm_launch_opts.no_fuse: the lone kernel, both stores written through) and to dpm_plan_run -- at the bench's size,
at a ragged request count, and at a tile count that is no multiple of the XCD split.  Every trajectory runs the forms
the store policy touches: LIN1 with the m store (first stage), TWO (steady state), LIN1 without it (lower_order_final).
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
from dpm_solver_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CODE = {torch.float16: L.DTYPE_F16, torch.bfloat16: L.DTYPE_BF16}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    yield
    torch.cuda.synchronize()


def _schedule():
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))


def _requests(n_req, shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    reqs = []
    for _ in range(n_req):
        x_T = torch.randn(shape, generator=g).to(DEV, dt)
        e0 = torch.randn(shape, generator=g).to(DEV, dt)
        xb = [x_T] + [torch.empty_like(x_T) for _ in range(3)]
        hb = [torch.empty_like(x_T) for _ in range(3)]
        rb = L.RunBuffers()
        for i in range(4):
            rb.xbuf[i] = xb[i].data_ptr()
        for i in range(3):
            rb.hist[i] = hb[i].data_ptr()
        rb.e0 = e0.data_ptr()
        rb.n, rb.batch = x_T.numel(), shape[0]
        rb.state_dtype, rb.eps_dtype = _CODE[dt], _CODE[dt]
        reqs.append(dict(rb=rb, x=xb, h=hb, e0=e0))
    return reqs


def _run(plan, reqs, no_fuse):
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = len(reqs)
    opts = L.LaunchOpts()
    opts.no_fuse = 1 if no_fuse else 0
    for r in reqs:
        for b in r["x"][1:] + r["h"]:
            b.fill_(float("nan"))
        r["rb"].opts = C_.pointer(opts)
    rbs = (L.RunBuffers * n)(*[r["rb"] for r in reqs])
    res = (C_.c_int * n)()
    try:
        L.check(L.lib.dpm_plan_run_multi(plan.handle, rbs, n, stream, None, res))
        torch.cuda.synchronize()
    finally:
        for r in reqs:
            r["rb"].opts = None
    return [reqs[i]["x"][res[i]].clone() for i in range(n)]


def _plan(dt, steps):
    ns = _schedule()
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: x, ns), ns, algorithm_type="dpmsolver++", state_dtype=dt)
    return dpm._get_plan(method="multistep", order=2, steps=steps, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N)


@pytest.mark.parametrize("n_req,shape,dt,steps", [
    (32, (256, 4, 64, 64), torch.float16, 5),      # the bench's launch: 65 536 tiles
    (7, (256, 4, 64, 64), torch.float16, 4),       # a ragged request count
    (5, (3, 4, 33, 40), torch.float16, 6),         # 8 tiles per request (7.7 rounded up): 40 tiles, no multiple of 8 per XCD
    (3, (1, 3, 56, 56), torch.float16, 6),         # 5 tiles per request, the last one partial
    (6, (16, 4, 64, 64), torch.bfloat16, 5),
])
def test_fused_store_policy_keeps_the_bits(n_req, shape, dt, steps):
    plan = _plan(dt, steps)
    reqs = _requests(n_req, shape, dt, seed=11 + n_req)
    fused = _run(plan, reqs, no_fuse=False)
    lone = _run(plan, reqs, no_fuse=True)
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    r1 = C_.c_int(-1)
    for i in (0, n_req - 1):
        rb = reqs[i]["rb"]
        L.check(L.lib.dpm_plan_run(plan.handle, C_.byref(rb), None, None, stream, C_.byref(r1)))
        torch.cuda.synchronize()
        assert torch.equal(fused[i], reqs[i]["x"][r1.value]), "request %d: fused launch vs dpm_plan_run" % i
    for i, (a, b) in enumerate(zip(fused, lone)):
        assert bool(torch.isfinite(a.float()).all()), "request %d: non-finite state" % i
        assert torch.equal(a, b), "request %d: fused launch vs one launch per request" % i
