"""The two-condition stage kernel (DPM_GUIDE_CFG2, stage_pair_kernel) through the C ABI on guard-banded arenas
(tests/pair_guarded.py), bit for bit against its numpy double (tests/pair_double.py).  Sizes sit on the kernel's own edges: 1 the
smallest, 7 below one group, 8 one group, 2040 / 2048 / 2056 one group below, on and above a tile, 4100 ragged past two tiles;
2048 and 4100 again one element past the 16-byte boundary (one element per lane).  The kernel loops over a capped grid: one case
per state width at the smallest n tests/grid_plan.py says takes a second iteration, and one on the one-element-per-lane route.
Three anchors need no double.  Run on an MI355X:  pytest -m gpu
"""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import grid_plan as GP
import guarded as G
import pair_guarded as PG
from dpm_solver_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 7, 8, 2040, 2048, 2056, 4100]
BATCHES = [1, 3]
OFFSET1 = [2048, 4100]                         # ... also one element past the 16-byte boundary: one element per lane
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
         (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)]
PAIR_IDS = ["%s-%s" % (G._name(s), G._name(e)) for s, e in PAIRS]
FORMS = {"LIN1": (L.FORM_LIN1, 0), "TWO": (L.FORM_TWO, 0), "TWO_BH": (L.FORM_TWO, L.F_BASE_HIST), "MS3": (L.FORM_MS3, 0),
         "SS3T": (L.FORM_SS3T, 0), "DENOISE": (L.FORM_DENOISE, 0)}
MODELS = ("noise", "v", "x_start", "score")
SCALES = ((7.5, 1.5), (1.5, -6.0), (1.0, 2.5))  # (s1, s2): composable, InstructPix2Pix's s_T = 7.5 / s_I = 1.5, guidance_scale 1
PER_CELL = 3
PAIR, CFG, NONE = L.GUIDE["classifier-free-2"], L.GUIDE["classifier-free"], L.GUIDE["uncond"]


def variants():
    """form x model type x DPM_F_TO_X0, with STORE_M and the scales in rotation: 48"""
    out = []
    for i, form in enumerate(FORMS):
        for j, model in enumerate(MODELS):
            for k, tox0 in enumerate((True, False)):
                out.append(dict(form=form, model=model, tox0=tox0, store_m=(i + j + k) % 2 == 0, s=SCALES[(i + 2 * j + k) % 3]))
    return out


def plan(pair_index, batch):
    """[(P, offset, variant)] of one (dtype pair, batch): every size with PER_CELL variants in rotation, the offset cells too"""
    vs = variants()
    random.Random(41 * pair_index + batch).shuffle(vs)
    cells = [(P, 0) for P in SIZES] + [(P, 1) for P in OFFSET1]
    return [(P, off, vs[(PER_CELL * i + j) % len(vs)]) for i, (P, off) in enumerate(cells) for j in range(PER_CELL)]


def route_of(n, offset):
    return "vec" if n % 8 == 0 and offset == 0 else "lane"


def test_table_meets_the_coverage_rule():
    vs = variants()
    assert len(vs) == 48 and SIZES == [1, 7, 8, 2040, 2048, 2056, 4100] and OFFSET1 == [2048, 4100] and BATCHES == [1, 3]
    assert len(set(PAIRS)) == 5
    for key, vals in (("form", set(FORMS)), ("model", set(MODELS))):
        for val in vals:
            mine = [v for v in vs if v[key] == val]
            assert {v["tox0"] for v in mine} == {True, False} and {v["store_m"] for v in mine} == {True, False}
            assert {v["s"] for v in mine} == set(SCALES)
    met = {}
    for p in range(len(PAIRS)):
        for batch in BATCHES:
            pl = plan(p, batch)
            assert {(P, off) for P, off, _ in pl} == {(P, 0) for P in SIZES} | {(P, 1) for P in OFFSET1}
            for P, off, v in pl:
                met.setdefault(route_of(P * batch, off), set()).update({v["form"], v["model"], ("pair", p), ("tox0", v["tox0"])})
    every = set(FORMS) | set(MODELS) | {("pair", p) for p in range(5)} | {("tox0", True), ("tox0", False)}
    assert set(met) == {"vec", "lane"}
    assert all(m == every for m in met.values()), {k: every - m for k, m in met.items()}


def make_stage(v, seed=0, extra_flags=0, guidance=PAIR):
    """a stage record with scalars of realistic magnitude"""
    rng = random.Random(seed)
    st = L.Stage()
    form, fflags = FORMS[v["form"]] if v["form"] in FORMS else (L.FORM_UNIPC, 0)
    st.index, st.form, st.model_type, st.guidance = 3, form, L.MODEL[v["model"]], guidance
    st.flags = (L.F_TO_X0 if v["tox0"] else 0) | (L.F_STORE_M if v["store_m"] else 0) | fflags | extra_flags
    st.h1_slot = st.h2_slot = st.m_slot = -1
    a = rng.uniform(0.05, 0.999)
    st.alpha_e, st.sigma_e = a, math.sqrt(1.0 - a * a)
    st.cfg_scale, st.cg_scale = v["s"]
    st.thr_ratio, st.thr_max = 0.995, 1.0
    st.blend_alpha, st.blend_sigma = 0.8, 0.6
    st.cx, st.c0, st.c1, st.c2 = (rng.uniform(-2, 2) for _ in range(4))
    for j in range(4):
        st.k[j] = rng.uniform(-1.5, 1.5)
    st.k[4] = rng.uniform(0.5, 1.5)
    return st


class _Pristine:
    def __init__(self, pristine):
        self.pristine = pristine


def make_case(v, P, batch, sd, ed, offset=0, seed=0, req=0, like=None, per_request=False, outputs=None, **kw):
    """outputs: None -- three independent normal outputs; else f(e0, e1, g) -> (e0, e1, g) on the drawn bit patterns"""
    st = make_stage(v, seed * 131 + req, kw.pop("extra_flags", 0))
    mk = lambda lk: PG.PairLaunch("pair", st, P * batch, sd, ed, batch=batch, offset=offset, like=lk,
                                  sep_xe=v["form"] in ("SS3T", "TWO_BH"), seed=seed, req=req, per_request_stages=per_request, **kw)
    case = mk(like)
    if outputs is None or like is not None:
        return case
    pr = dict(case.pristine)
    pr["e0"], pr["e1"], pr["g"] = outputs(pr["e0"], pr["e1"], pr["g"])
    return mk(_Pristine(pr))


def other_guidance(case, v, guidance, e0=None):
    """the same operands under DPM_GUIDE_CFG (e0, e1) or unguided (on `e0` of the pair case's pristine operands)"""
    st = make_stage(v, 0, 0, guidance)
    C.memmove(C.byref(st), C.byref(case.st), C.sizeof(L.Stage))
    st.guidance = guidance
    pr = dict(case.pristine)
    if e0 is not None:
        pr["e0"] = pr[e0]
    kw = dict(case.kw)
    return G.GuardedLaunch("plain", st, case.n, case.sd, case.ed, like=_Pristine(pr), **kw)


def sweep_case(pair, batch, i, P, off, v):
    sd, ed = PAIRS[pair]
    return make_case(v, P, batch, sd, ed, offset=off, seed=100 * pair + i)


@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=PAIR_IDS)
def test_the_double_stays_inside_its_payloads(pair):
    """the doubles of the whole sweep on the CPU: every output element written, no guard touched, no input changed"""
    for batch in BATCHES:
        for i, (P, off, v) in enumerate(plan(pair, batch)):
            PG.run_double(sweep_case(pair, batch, i, P, off, v))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(dev):
    rc = L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), _stream())
    torch.cuda.synchronize()
    return rc


def run_case(case):
    want, dev = PG.run_double(case), case.on(DEV)
    rc = launch(dev)
    assert rc == 0, (rc, L.lib.dpm_last_error())
    dev.verify(want)
    return dev


@gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=PAIR_IDS)
def test_sizes_forms_and_network_kinds(pair, batch):
    for i, (P, off, v) in enumerate(plan(pair, batch)):
        try:
            run_case(sweep_case(pair, batch, i, P, off, v))
        except AssertionError as e:
            raise AssertionError("P=%d batch=%d offset=%d %s: %s" % (P, batch, off, v, e)) from e


def device_cu():
    n, lds = C.c_int(0), C.c_int(0)
    L.check(L.lib.dpm_device_info(C.byref(n), C.byref(lds), C.create_string_buffer(64), 64))
    return n.value


@gpu
@pytest.mark.parametrize("sd", [torch.float16, torch.float32], ids=["2-byte", "4-byte"])
def test_the_smallest_launch_whose_tile_walk_takes_a_second_iteration(sd):
    """the 16-byte route's grid is the streaming family's (stream_grid_plan, one tile per iteration), capped per CU: K + 1 tiles
    whole tiles and one more 8-element group is the smallest launch in which a 256-lane group walks two tiles"""
    n_cu = device_cu()
    n = GP.gates(n_cu)["K"] * GP.T + 8
    assert GP.route(n, n_cu)["trips"] == 2 and GP.route(n - 8, n_cu)["trips"] == 1
    v = dict(form="TWO", model="noise", tox0=True, store_m=True, s=(7.5, 1.5))
    run_case(make_case(v, n, 1, sd, sd, seed=77))


@gpu
def test_the_smallest_launch_whose_lanes_loop_on_the_scalar_route():
    n_cu = device_cu()
    n = GP.gates(n_cu)["S"] + 1                                              # (odd: one element per lane)
    assert GP.route(n, n_cu)["scalar_trips"] == 2 and n % 8 != 0
    v = dict(form="MS3", model="v", tox0=True, store_m=True, s=(1.5, -6.0))
    run_case(make_case(v, n, 1, torch.float32, torch.float16, seed=78))


# ------------------------------------------------------------------------------------------------
# anchors that do not depend on the double
# ------------------------------------------------------------------------------------------------
def _gpu_bits(case):
    dev = case.on(DEV)
    rc = launch(dev)
    assert rc == 0, (rc, L.lib.dpm_last_error())
    dev.verify()
    return {name: dev.arenas[name].payload_bits().cpu() for name in dev.written}


ANCHOR_SIZES = [(7, 3, 0), (2048, 3, 0), (2056, 1, 0), (4100, 2, 0), (2048, 1, 1)]
ANCHOR_FORMS = [("TWO", "noise", False), ("MS3", "v", True), ("SS3T", "x_start", False), ("DENOISE", "score", True)]


@gpu
@pytest.mark.parametrize("form,model,tox0", ANCHOR_FORMS)
@pytest.mark.parametrize("P,batch,off", ANCHOR_SIZES)
def test_fp32_outputs_with_a_zero_s2_are_the_classifier_free_launch(P, batch, off, form, model, tox0):
    """s2 == 0: s2 * d2 is a zero (d2 is finite), and adding a zero changes no non-zero bit; a sum that is itself a zero keeps
    its sign unless it is -0 next to +0 -- which (n1 + s1 * d0) == -0 would need, and the draws do not produce"""
    f32 = torch.float32
    v = dict(form=form, model=model, tox0=tox0, store_m=True, s=(7.5, 0.0))
    pair = make_case(v, P, batch, f32, f32, offset=off, seed=51)
    got, want = _gpu_bits(pair), _gpu_bits(other_guidance(pair, v, CFG))
    assert set(got) == set(want) == {"x_out", "m_out"}
    for name in got:
        assert torch.equal(got[name], want[name]), name


@gpu
@pytest.mark.parametrize("form,model,tox0", ANCHOR_FORMS)
@pytest.mark.parametrize("P,batch,off", ANCHOR_SIZES)
def test_fp32_outputs_with_g_equal_to_e1_are_the_classifier_free_launch(P, batch, off, form, model, tox0):
    """g == e1: n2 == n1 bit for bit, d2 = +0, s2 * d2 a zero -- the classifier-free blend's own three operations, then a zero"""
    f32 = torch.float32
    v = dict(form=form, model=model, tox0=tox0, store_m=True, s=(7.5, 1.5))
    pair = make_case(v, P, batch, f32, f32, offset=off, seed=53, outputs=lambda e0, e1, g: (e0, e1, e1.clone()))
    got, want = _gpu_bits(pair), _gpu_bits(other_guidance(pair, v, CFG))
    for name in ("x_out", "m_out"):
        assert torch.equal(got[name], want[name]), name


@gpu
@pytest.mark.parametrize("sd,ed", [PAIRS[0], PAIRS[1], PAIRS[3], PAIRS[4]], ids=[PAIR_IDS[i] for i in (0, 1, 3, 4)])
@pytest.mark.parametrize("P,batch,off", ANCHOR_SIZES)
def test_three_equal_outputs_on_a_data_prediction_stage_are_the_unguided_launch(P, batch, off, sd, ed):
    """e0 == e1 == g: both differences are +0 and eps = n1 up to the sign of a zero, which x0 = (xe - sigma * eps) / alpha does
    not see; under DPM_F_TO_X0 the unguided launch has fp32 model values as well"""
    for form, model in (("TWO", "noise"), ("MS3", "v")):
        v = dict(form=form, model=model, tox0=True, store_m=True, s=(7.5, 1.5))
        pair = make_case(v, P, batch, sd, ed, offset=off, seed=57, outputs=lambda e0, e1, g: (e1.clone(), e1, e1.clone()))
        got, want = _gpu_bits(pair), _gpu_bits(other_guidance(pair, v, NONE, e0="e1"))
        for name in ("x_out", "m_out"):
            assert torch.equal(got[name], want[name]), (form, name)


# ------------------------------------------------------------------------------------------------
# errors, multi-request launches
# ------------------------------------------------------------------------------------------------
BAD = {
    "thresholding": (dict(extra_flags=L.F_THRESH), {}, L.ERR_UNSUPPORTED),
    "blend": (dict(extra_flags=L.F_BLEND, blend=(8, True)), {}, L.ERR_UNSUPPORTED),
    "noise": (dict(extra_flags=L.F_NOISE), {}, L.ERR_UNSUPPORTED),
    "user_x0": (dict(extra_flags=L.F_USER_X0), {}, L.ERR_UNSUPPORTED),
    "unipc": ({}, dict(form="UNIPC"), L.ERR_UNSUPPORTED),
    "x_out2": (dict(dup=True), {}, L.ERR_UNSUPPORTED),
    "stride": (dict(eps_stride=2048 + 64), {}, L.ERR_UNSUPPORTED),
    "double": (dict(f64=True), {}, L.ERR_UNSUPPORTED),
    "rescale": (dict(extra_flags=L.F_CFG_RESCALE), {}, L.ERR_ARG),
    "apg": (dict(extra_flags=L.F_CFG_APG), {}, L.ERR_ARG),
    "zstar": (dict(extra_flags=L.F_CFG_ZSTAR), {}, L.ERR_ARG),
    "no_e1": (dict(without=("e1",)), {}, L.ERR_ARG),
    "no_g": (dict(without=("g",)), {}, L.ERR_ARG),
    "nan_s1": ({}, dict(s=(float("nan"), 1.5)), L.ERR_ARG),
    "inf_s2": ({}, dict(s=(7.5, float("inf"))), L.ERR_ARG),
    "form": (dict(form_code=9), {}, L.ERR_ARG),
}


@gpu
@pytest.mark.parametrize("what", sorted(BAD))
def test_error_returns_write_nothing(what):
    kw, vkw, code = BAD[what]
    kw = dict(kw)
    form_code, eps_stride, f64 = kw.pop("form_code", None), kw.pop("eps_stride", 0), kw.pop("f64", False)
    v = dict(dict(form="LIN1", model="noise", tox0=True, store_m=True, s=(7.5, 1.5)), **vkw)
    dt = torch.float64 if f64 else torch.float16
    dev = make_case(v, 2048, 3, dt, dt, seed=3, **kw).on(DEV)
    if form_code is not None:
        dev.st.form = form_code
    dev.b.eps_stride = eps_stride
    rc = launch(dev)
    assert rc == code, (rc, L.lib.dpm_last_error())
    assert b"DPM_GUIDE_CFG2" in L.lib.dpm_last_error() or what in ("form", "rescale", "apg", "zstar")
    dev.verify(rc=rc)
    # ... and as the last request of a multi-request call, in every mode, behind a well-formed one that must not run either
    ok = make_case(dict(v, form="LIN1", s=(7.5, 1.5)), 2048, 3, dt if not f64 else torch.float16, dt if not f64 else torch.float16,
                   seed=4, per_request=True).on(DEV)
    st, bs = (L.Stage * 2)(ok.st, dev.st), (L.Buffers * 2)(ok.b, dev.b)
    for per_request in (0, 1):
        ok.opts.per_request_stages = per_request
        rc2 = L.lib.dpm_stage_launch_multi(st if per_request else C.byref(dev.st), bs, 2, _stream())
        torch.cuda.synchronize()
        assert rc2 == code, (per_request, rc2, L.lib.dpm_last_error())
        dev.verify(rc=rc2)
        ok.verify(rc=rc2)


def _plain_case(form, P, batch, sd, ed, seed, req):
    """a classifier-free request the fused and the table launches take"""
    v = dict(form=form, model="noise", tox0=True, store_m=True, s=(7.5, 0.0))
    st = make_stage(v, seed * 131 + req, 0, CFG)
    return G.GuardedLaunch("plain", st, P * batch, sd, ed, batch=batch, seed=seed, req=req, per_request_stages=True)


def _run_plain_double(case):
    assert G.double_launch(case.st, case.b) == 0
    case.verify()
    return case


@gpu
@pytest.mark.parametrize("mode", ["per_request", "fuse_shapes", "table"])
def test_a_pair_request_in_a_multi_request_call_runs_on_its_own(mode):
    """five requests with per-request stages, the second and the fourth two-condition ones between three classifier-free ones
    that fuse: each gets the bits of its double and of its own lone launch -- with per-request stages, with fuse_shapes as
    well, and in a table call (DPM_TABLE_FILL on the host, then DPM_TABLE_LAUNCH)"""
    sd = ed = torch.float16
    P, batch = 2048, 2
    pv = dict(model="noise", tox0=True, store_m=True, s=(7.5, 1.5))
    cases = [_plain_case("TWO", P, batch, sd, ed, 21, 0), make_case(dict(pv, form="MS3"), P, batch, sd, ed, seed=21, req=1, per_request=True),
             _plain_case("LIN1", P, batch, sd, ed, 21, 2), make_case(dict(pv, form="TWO"), P, batch, sd, ed, seed=21, req=3, per_request=True),
             _plain_case("TWO", P, batch, sd, ed, 21, 4)]
    is_pair = [c.st.guidance == PAIR for c in cases]
    wants = [PG.run_double(c) if p else _run_plain_double(c) for c, p in zip(cases, is_pair)]
    devs = [c.on(DEV) for c in cases]
    st = (L.Stage * 5)(*[d.st for d in devs])
    bs = (L.Buffers * 5)(*[d.b for d in devs])
    if mode == "fuse_shapes":
        devs[0].opts.fuse_shapes = 1
    if mode == "table":
        nbytes = L.table_bytes(5)
        host = np.zeros(nbytes + 16, dtype=np.uint8)
        off = (-host.ctypes.data) % 16
        devs[0].opts.table_mode = L.TABLE_FILL
        bs[0].workspace = host.ctypes.data + off
        assert L.lib.dpm_stage_launch_multi(st, bs, 5, _stream()) == 0, L.lib.dpm_last_error()
        assert [int(w) for w in host[off:off + 16].view(np.uint32)][2:] == [5, 0]          # five requests, no run of rows
        tab = torch.from_numpy(host[off:off + nbytes].copy()).to(DEV)
        devs[0].opts.table_mode = L.TABLE_LAUNCH
        bs[0].workspace = tab.data_ptr()
    rc = L.lib.dpm_stage_launch_multi(st, bs, 5, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants)
    for r in (1, 3):
        lone = cases[r].on(DEV)
        assert launch(lone) == 0
        for name in ("x_out", "m_out"):
            assert torch.equal(lone.arenas[name].payload_bits(), devs[r].arenas[name].payload_bits()), (r, name)


@gpu
def test_lockstep_multi_launches_pair_requests_one_by_one():
    """dpm_stage_launch_multi with ONE stage record (mode 0: every request shares it, so every request is a two-condition one):
    no fused variant, three launches, each request the bits of its double and of its lone launch"""
    sd, ed = torch.float32, torch.bfloat16
    v = dict(form="TWO", model="v", tox0=True, store_m=True, s=(1.5, -6.0))
    cases = [make_case(v, 4100, 2, sd, ed, seed=33, req=r) for r in range(3)]
    for c in cases[1:]:
        C.memmove(C.byref(c.st), C.byref(cases[0].st), C.sizeof(L.Stage))
    wants, devs = [PG.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    bs = (L.Buffers * 3)(*[d.b for d in devs])
    rc = L.lib.dpm_stage_launch_multi(C.byref(devs[0].st), bs, 3, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants)
    for c, d in zip(cases, devs):
        lone = c.on(DEV)
        assert launch(lone) == 0
        for name in ("x_out", "m_out"):
            assert torch.equal(lone.arenas[name].payload_bits(), d.arenas[name].payload_bits()), name
