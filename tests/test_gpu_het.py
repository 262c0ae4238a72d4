"""GPU tests of the heterogeneous fused launch (dpm_stage_launch_multi with dpm_launch_opts.per_request_stages = 1):
request r advanced by its own stage record st[r] must end bit-identical to one dpm_stage_launch per request -- random
mixes of first-order / TWO / MS3 records, mixed STORE_M, classifier-free guidance with its duplicate store, x_start / v
networks (generic prologue), every dtype pair, ragged request counts and requests the fused kernel does not take
(thresholded, unaligned, separate evaluation state).  Run on an MI355X:  pytest -m gpu
"""
import ctypes as C_
import math
import random

import numpy as np
import pytest
import torch

from dpm_solver_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CODE = {torch.float16: L.DTYPE_F16, torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16}
PAIRS = [(torch.float16, torch.float16), (torch.float32, torch.float32), (torch.float32, torch.float16),
         (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    yield
    torch.cuda.synchronize()


def _stage(rng, form, model_type, guidance, to_x0, store_m):
    st = L.Stage()
    st.form, st.model_type, st.guidance = form, model_type, guidance
    st.flags = (L.F_TO_X0 if to_x0 else 0) | (L.F_STORE_M if store_m else 0)
    if form == L.FORM_TWO and rng.random() < 0.3:
        st.flags |= L.F_BASE_HIST
    a = rng.uniform(0.05, 0.999)
    st.alpha_e, st.sigma_e = a, math.sqrt(1.0 - a * a)
    st.cfg_scale = 3.0 if guidance == L.GUIDE["classifier-free"] else 1.0
    st.cx, st.c0, st.c1, st.c2 = (rng.uniform(-2, 2) for _ in range(4))
    for j in range(4):
        st.k[j] = rng.uniform(-1.5, 1.5)
    st.thr_ratio, st.thr_max = 0.995, 1.0
    return st


class Req:
    """one request's operands; `offset` elements in front of every buffer (offset 1: unaligned)"""

    def __init__(self, g, shape, sd, ed, cfg, offset=0, sep_xe=False):
        n = int(np.prod(shape))
        self.n, self.batch, self.sd, self.ed = n, shape[0], sd, ed

        def buf(dt, count=n, fill=True):
            t = torch.empty(count + offset, dtype=dt, device=DEV)
            v = t[offset:]
            if fill:
                v.copy_(torch.randn(count, generator=g).to(dt))
            return v
        self.x, self.e0, self.h1, self.h2 = buf(sd), buf(ed), buf(sd), buf(sd)
        self.e1 = buf(ed) if cfg else None
        self.xe = buf(sd) if sep_xe else None
        self.cfg = cfg
        self.ws = None

    def buffers(self, out):
        b = L.Buffers()
        b.x, b.e0, b.h1, b.h2 = (t.data_ptr() for t in (self.x, self.e0, self.h1, self.h2))
        if self.xe is not None:
            b.xe = self.xe.data_ptr()
        if self.e1 is not None:
            b.e1 = self.e1.data_ptr()
        b.x_out, b.m_out = out["x"].data_ptr(), out["m"].data_ptr()
        if self.cfg:
            b.x_out2 = out["x2"].data_ptr()
        b.n, b.batch = self.n, self.batch
        b.state_dtype, b.eps_dtype = _CODE[self.sd], _CODE[self.ed]
        if self.ws is not None:
            b.workspace = self.ws.data_ptr()
        return b

    def outputs(self, offset=0):
        def nan(count):
            t = torch.full((count + offset,), float("nan"), dtype=self.sd, device=DEV)
            return t[offset:]
        return dict(x=nan(self.n), m=nan(self.n), x2=nan(self.n))


def run_both(sts, reqs, offsets, no_fuse=False):
    """(per-request-stage multi launch, one dpm_stage_launch per request): their outputs"""
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    R = len(reqs)
    outs_m = [q.outputs(o) for q, o in zip(reqs, offsets)]
    outs_s = [q.outputs(o) for q, o in zip(reqs, offsets)]
    arr_st = (L.Stage * R)(*sts)
    arr_b = (L.Buffers * R)(*[q.buffers(o) for q, o in zip(reqs, outs_m)])
    opts = L.LaunchOpts()
    opts.per_request_stages = 1
    opts.no_fuse = 1 if no_fuse else 0
    arr_b[0].opts = C_.pointer(opts)
    L.check(L.lib.dpm_stage_launch_multi(arr_st, arr_b, R, stream))
    torch.cuda.synchronize()
    for r, q in enumerate(reqs):
        b = q.buffers(outs_s[r])
        L.check(L.lib.dpm_stage_launch(C_.byref(sts[r]), C_.byref(b), stream))
    torch.cuda.synchronize()
    return outs_m, outs_s


def check(sts, reqs, outs_m, outs_s):
    for r, (st, q, a, b) in enumerate(zip(sts, reqs, outs_m, outs_s)):
        assert torch.equal(a["x"], b["x"]), "request %d (form %d flags %d)" % (r, st.form, st.flags)
        assert torch.isfinite(a["x"].float()).all()
        if st.flags & L.F_STORE_M:
            assert torch.equal(a["m"], b["m"]), "request %d: model value" % r
        else:
            assert torch.isnan(a["m"].float()).all(), "request %d: m_out written without STORE_M" % r
        if q.cfg:
            assert torch.equal(a["x2"], a["x"]) and torch.equal(b["x2"], b["x"]), "request %d: duplicate store" % r


def _mix(n_req, sd, ed, seed, cfg=False, model_type="noise", to_x0=True, mixed_groups=False, unfusable=0,
         shape=(2, 4, 24, 32)):
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    sts, reqs, offsets = [], [], []
    for r in range(n_req):
        mt, tx = L.MODEL[model_type], to_x0
        if mixed_groups:                          # several groups in one call: other model types / conversions
            mt = rng.choice([L.MODEL["noise"], L.MODEL["x_start"], L.MODEL["v"]])
            tx = rng.random() < 0.6
        form = rng.choice([L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3])
        st = _stage(rng, form, mt, L.GUIDE["classifier-free"] if cfg else L.GUIDE["uncond"], tx, rng.random() < 0.6)
        kind = "plain" if r >= unfusable else ("thresh", "unaligned", "xe")[r % 3]
        off = 1 if kind == "unaligned" else 0
        q = Req(g, shape, sd, ed, cfg, offset=off, sep_xe=kind == "xe")
        if kind == "thresh":
            st.flags |= L.F_THRESH | L.F_TO_X0
            nb = L.lib.dpm_threshold_workspace_bytes(q.batch, q.n // q.batch)
            if nb:
                q.ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        if kind == "xe":
            st.flags |= L.F_TO_X0
        sts.append(st)
        reqs.append(q)
        offsets.append(off)
    return sts, reqs, offsets


@pytest.mark.parametrize("sd,ed", PAIRS)
@pytest.mark.parametrize("n_req", [1, 7, 32, 33])
def test_het_equals_single(sd, ed, n_req):
    sts, reqs, offs = _mix(n_req, sd, ed, seed=n_req * 11 + _CODE[sd] * 3 + _CODE[ed])
    check(sts, reqs, *run_both(sts, reqs, offs))


@pytest.mark.parametrize("sd,ed", PAIRS)
def test_het_cfg_duplicate_store(sd, ed):
    sts, reqs, offs = _mix(9, sd, ed, seed=5, cfg=True)
    check(sts, reqs, *run_both(sts, reqs, offs))


@pytest.mark.parametrize("sd,ed", [(torch.float16, torch.float16), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("model_type,to_x0,cfg", [("x_start", True, False), ("v", True, True), ("noise", False, False),
                                                 ("noise", False, True), ("v", False, False)])
def test_het_generic_prologue(sd, ed, model_type, to_x0, cfg):
    sts, reqs, offs = _mix(12, sd, ed, seed=17, cfg=cfg, model_type=model_type, to_x0=to_x0)
    check(sts, reqs, *run_both(sts, reqs, offs))


@pytest.mark.parametrize("sd,ed", PAIRS)
def test_het_mixed_groups_and_unfusable(sd, ed):
    """requests of several groups (model type, conversion) and requests the fused kernel does not take, interleaved"""
    sts, reqs, offs = _mix(21, sd, ed, seed=23, mixed_groups=True, unfusable=6)
    check(sts, reqs, *run_both(sts, reqs, offs))


def test_het_no_fuse_and_ragged():
    """no_fuse launches request by request; a ragged size (n % 8 != 0) is not fused either -- same bits"""
    sts, reqs, offs = _mix(5, torch.float16, torch.float16, seed=3)
    check(sts, reqs, *run_both(sts, reqs, offs, no_fuse=True))
    sts, reqs, offs = _mix(5, torch.float32, torch.float32, seed=4, shape=(3, 5, 7))
    check(sts, reqs, *run_both(sts, reqs, offs))


def test_het_reports_request_errors():
    sts, reqs, offs = _mix(3, torch.float16, torch.float16, seed=1)
    outs = [q.outputs() for q in reqs]
    arr_b = (L.Buffers * 3)(*[q.buffers(o) for q, o in zip(reqs, outs)])
    arr_b[2].h1 = None
    sts[2].form = L.FORM_TWO
    opts = L.LaunchOpts()
    opts.per_request_stages = 1
    arr_b[0].opts = C_.pointer(opts)
    rc = L.lib.dpm_stage_launch_multi((L.Stage * 3)(*sts), arr_b, 3, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and b"needs h1" in L.lib.dpm_last_error()
    assert all(torch.isnan(o["x"].float()).all() for o in outs)      # nothing launched
