"""The CFG-Zero* stage kernel (DPM_F_CFG_ZSTAR, stage_zstar_kernel) through the C ABI on guard-banded arenas (tests/guarded.py),
bit for bit against its numpy double (tests/zstar_double.py, whose inputs are checked decidable on the CPU first: a does not
depend on the summation order).  Sample sizes sit on the kernel's own edges: 1 the smallest legal, 7 and 4100 ragged (one
element per lane), 8 one group, 2048 a partial iteration, 16384 the last size whose outputs stay in registers, 16392 the first
that reads them twice.  Half of the cases draw independent normal outputs, half o_c = 0.8 o_u + 0.6 z (a near 0 and near 0.8).
Three anchors need no double: e1 == 0, e0 == e1 and e0 == 2 e1.  Run on an MI355X:  pytest -m gpu
"""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import guarded as G
import kernel_double as KD
import zstar_double as ZD
from dpm_solver_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 7, 8, 2048, 4100, 16384, 16392]
BATCHES = [1, 3]
OFFSET1 = [2048, 16392]                       # ... also one element past the 16-byte boundary: one element per lane, both paths
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
         (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)]
PAIR_IDS = ["%s-%s" % (G._name(s), G._name(e)) for s, e in PAIRS]
FORMS = {"LIN1": (L.FORM_LIN1, 0), "TWO": (L.FORM_TWO, 0), "TWO_BH": (L.FORM_TWO, L.F_BASE_HIST), "MS3": (L.FORM_MS3, 0),
         "SS3T": (L.FORM_SS3T, 0), "DENOISE": (L.FORM_DENOISE, 0)}
MODELS = ("noise", "v", "x_start", "score")
SCALES = (7.5, 1.5)
PER_CELL = 3


def variants():
    """form x model type x DPM_F_TO_X0, with STORE_M, x_out2 and s in rotation: 48"""
    out = []
    for i, form in enumerate(FORMS):
        for j, model in enumerate(MODELS):
            for k, tox0 in enumerate((True, False)):
                out.append(dict(form=form, model=model, tox0=tox0, store_m=(i + j + k) % 2 == 0, dup=(i + 2 * j + k) % 3 != 0,
                                s=SCALES[(i + j // 2 + k) % 2]))
    return out


def plan(pair_index, batch):
    """[(P, offset, variant)] of one (dtype pair, batch): every size with PER_CELL variants in rotation, the offset cells too"""
    vs = variants()
    random.Random(37 * pair_index + batch).shuffle(vs)
    cells = [(P, 0) for P in SIZES] + [(P, 1) for P in OFFSET1]
    return [(P, off, vs[(PER_CELL * i + j) % len(vs)]) for i, (P, off) in enumerate(cells) for j in range(PER_CELL)]


def path_of(P, offset):
    return ("vec" if P % 8 == 0 and offset == 0 else "lane") + ("-keep" if P <= 16384 else "-reread")


def test_table_meets_the_coverage_rule():
    vs = variants()
    assert len(vs) == 48 and SIZES == [1, 7, 8, 2048, 4100, 16384, 16392] and BATCHES == [1, 3] and len(set(PAIRS)) == 5
    for key, vals in (("form", set(FORMS)), ("model", set(MODELS))):
        for val in vals:
            mine = [v for v in vs if v[key] == val]
            assert {v["tox0"] for v in mine} == {True, False} and {v["store_m"] for v in mine} == {True, False}
            assert {v["dup"] for v in mine} == {True, False} and {v["s"] for v in mine} == {7.5, 1.5}
    met = {}
    for p in range(len(PAIRS)):
        for batch in BATCHES:
            pl = plan(p, batch)
            assert {(P, off) for P, off, _ in pl} == {(P, 0) for P in SIZES} | {(P, 1) for P in OFFSET1}
            for P, off, v in pl:
                met.setdefault(path_of(P, off), set()).update({v["form"], v["model"], ("pair", p), ("tox0", v["tox0"])})
    every = set(FORMS) | set(MODELS) | {("pair", p) for p in range(5)} | {("tox0", True), ("tox0", False)}
    assert set(met) == {"vec-keep", "lane-keep", "vec-reread", "lane-reread"}
    assert all(m == every for m in met.values()), {k: every - m for k, m in met.items()}


def make_stage(v, seed=0, extra_flags=0, flag=True):
    """a flagged stage record with scalars of realistic magnitude"""
    rng = random.Random(seed)
    st = L.Stage()
    form, fflags = FORMS[v["form"]] if v["form"] in FORMS else (L.FORM_UNIPC, 0)
    st.index, st.form, st.model_type, st.guidance = 3, form, L.MODEL[v["model"]], L.GUIDE["classifier-free"]
    st.flags = ((L.F_TO_X0 if v["tox0"] else 0) | (L.F_STORE_M if v["store_m"] else 0) | fflags
                | (L.F_CFG_ZSTAR if flag else 0) | extra_flags)
    st.h1_slot = st.h2_slot = st.m_slot = -1
    a = rng.uniform(0.05, 0.999)
    st.alpha_e, st.sigma_e = a, math.sqrt(1.0 - a * a)
    st.cfg_scale, st.cg_scale = v["s"], v["s"] * st.sigma_e                    # (cg_scale: the planner's, read by nothing here)
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


def _bits(values, dt):
    t = values.to(dt)
    return t.view(G._INT[t.element_size()])


def _values(bits, dt):
    return bits.view(dt).float()


def make_case(v, P, batch, sd, ed, offset=0, seed=0, req=0, like=None, per_request=False, outputs=None, flag=True, **kw):
    """outputs: None -- independent normal e0 / e1 (guarded.py's own draw); else f(e0, e1) -> (e0, e1) on fp32 tensors of the
    drawn values, stored in the network's dtype"""
    st = make_stage(v, seed * 131 + req, kw.pop("extra_flags", 0), flag)
    mk = lambda lk: G.GuardedLaunch("zstar", st, P * batch, sd, ed, batch=batch, offset=offset, dup=v["dup"],
                                    sep_xe=v["form"] in ("SS3T", "TWO_BH"), seed=seed, req=req, like=lk,
                                    per_request_stages=per_request, **kw)
    case = mk(like)
    if outputs is None or like is not None:
        return case
    pr = dict(case.pristine)
    e0, e1 = outputs(_values(pr["e0"], ed), _values(pr["e1"], ed))
    pr["e0"], pr["e1"] = _bits(e0, ed), _bits(e1, ed)
    return mk(_Pristine(pr))


def correlated(e0, e1):
    return 0.8 * e1 + 0.6 * e0, e1


def run_double(case):
    assert ZD.launch_raw_double(KD._Ref(case.st), KD._Ref(case.b)) == 0      # (asserts the inputs decidable first)
    case.verify()
    return case


def sweep_case(pair, batch, i, P, off, v):
    sd, ed = PAIRS[pair]
    return make_case(v, P, batch, sd, ed, offset=off, seed=100 * pair + i, outputs=correlated if i % 2 else None)


@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=PAIR_IDS)
def test_inputs_of_every_case_are_decidable(pair):
    """the doubles of the whole sweep on the CPU: none of its samples has an a that depends on the summation order (the
    precondition under which the GPU tests may ask for equal bits), and the double stays inside its payloads"""
    for batch in BATCHES:
        for i, (P, off, v) in enumerate(plan(pair, batch)):
            run_double(sweep_case(pair, batch, i, P, off, v))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(dev):
    rc = L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), _stream())
    torch.cuda.synchronize()
    return rc


def run_case(case):
    want, dev = run_double(case), case.on(DEV)
    rc = launch(dev)
    assert rc == 0, (rc, L.lib.dpm_last_error())
    dev.verify(want)
    if "x_out2" in dev.written:                                               # (verify held both to the double; say it outright)
        a, b = dev.arenas["x_out"], dev.arenas["x_out2"]
        assert torch.equal(a.payload_bits(), b.payload_bits())
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


@gpu
@pytest.mark.parametrize("P", [7, 2048, 16392])
def test_a_sample_does_not_depend_on_the_batch_around_it(P):
    v = dict(form="TWO", model="v", tox0=True, store_m=True, dup=True, s=7.5)
    sd, ed = torch.float32, torch.float16
    whole = run_case(make_case(v, P, 3, sd, ed, seed=5, outputs=correlated))
    for k in range(3):
        one = _Pristine({name: bits[k * P:(k + 1) * P] for name, bits in whole.pristine.items()})
        alone = make_case(v, P, 1, sd, ed, seed=5, like=one)
        assert bytes(alone.st) == bytes(whole.st)
        dev = run_case(alone)
        for name in ("x_out", "m_out", "x_out2"):
            assert torch.equal(dev.arenas[name].payload_bits().cpu(), whole.arenas[name].payload_bits().cpu()[k * P:(k + 1) * P]), (name, k)


# ------------------------------------------------------------------------------------------------
# anchors that do not depend on the double: an fp32 noise network, DPM_F_TO_X0 off
# ------------------------------------------------------------------------------------------------
def _gpu_bits(case):
    dev = case.on(DEV)
    rc = launch(dev)
    assert rc == 0, (rc, L.lib.dpm_last_error())
    dev.verify()
    return dev, {name: dev.arenas[name].payload_bits().cpu() for name in dev.written}


ANCHOR_SIZES = [(7, 3), (2048, 3), (4100, 2), (16392, 2)]


@gpu
@pytest.mark.parametrize("P,batch", ANCHOR_SIZES)
def test_a_zero_unconditional_output_gives_s_times_the_conditional_one(P, batch):
    """S_uu == 0: a = 0, defined -- u = 0, g = 0 + s * (o_c - 0).  A DENOISE stage stores g itself."""
    f32 = torch.float32
    v = dict(form="DENOISE", model="noise", tox0=False, store_m=True, dup=True, s=7.5)
    case = make_case(v, P, batch, f32, f32, seed=41, outputs=lambda e0, e1: (e0, torch.zeros_like(e1)))
    dev, got = _gpu_bits(case)
    e0 = _values(case.pristine["e0"], f32)
    want = _bits(torch.tensor(7.5, dtype=f32) * e0, f32)
    for name in ("x_out", "m_out", "x_out2"):
        assert torch.equal(got[name], want), name


@gpu
@pytest.mark.parametrize("form", ["TWO", "MS3", "DENOISE"])
@pytest.mark.parametrize("P,batch", ANCHOR_SIZES)
def test_equal_outputs_give_the_flagless_stage(P, batch, form):
    """e0 == e1 with S_uu >= 1: a = fp32(S / (S + 1e-8)) = 1 (1e-8 / S <= 1e-8 < 2^-25), u = o_u, g = o_u + s * 0 -- the
    flag-less blend's own operations on the same operands"""
    f32 = torch.float32
    v = dict(form=form, model="noise", tox0=False, store_m=True, dup=True, s=7.5)
    same = lambda e0, e1: (e1, e1)
    flagged = make_case(v, P, batch, f32, f32, seed=43, outputs=same)
    e1 = _values(flagged.pristine["e1"], f32).double().reshape(batch, P)
    assert float((e1 * e1).sum(dim=1).min()) >= 1.0
    plain = make_case(v, P, batch, f32, f32, seed=43, outputs=same, flag=False)
    assert all(torch.equal(flagged.pristine[k], plain.pristine[k]) for k in flagged.pristine)
    _, got = _gpu_bits(flagged)
    _, want = _gpu_bits(plain)
    assert set(got) == set(want) == {"x_out", "m_out", "x_out2"}
    for name in got:
        assert torch.equal(got[name], want[name]), name


@gpu
@pytest.mark.parametrize("P,batch", ANCHOR_SIZES)
def test_a_doubled_conditional_output_does_not_depend_on_the_scale(P, batch):
    """e0 == 2 e1 with S_uu >= 1: a = 2, u = 2 o_u = o_c exactly, g = o_c + s * 0 for every s -- and the flag-less stage at
    s = 1 gives o_u + 1 * (o_c - o_u) = o_u + o_u = o_c as well"""
    f32 = torch.float32
    twice = lambda e0, e1: (2.0 * e1, e1)
    outs = []
    for s, flag in ((7.5, True), (1.5, True), (1.0, False)):
        v = dict(form="TWO", model="noise", tox0=False, store_m=True, dup=True, s=s)
        case = make_case(v, P, batch, f32, f32, seed=47, outputs=twice, flag=flag)
        e1 = _values(case.pristine["e1"], f32).double().reshape(batch, P)
        assert float((e1 * e1).sum(dim=1).min()) >= 1.0
        outs.append(_gpu_bits(case)[1])
    for name in ("x_out", "m_out", "x_out2"):
        assert torch.equal(outs[0][name], outs[1][name]) and torch.equal(outs[0][name], outs[2][name]), name


# ------------------------------------------------------------------------------------------------
# errors, multi-request launches
# ------------------------------------------------------------------------------------------------
BAD = {
    "thresholding": (dict(extra_flags=L.F_THRESH), {}, L.ERR_UNSUPPORTED),
    "blend": (dict(extra_flags=L.F_BLEND, blend=(8, True)), {}, L.ERR_UNSUPPORTED),
    "noise": (dict(extra_flags=L.F_NOISE), {}, L.ERR_UNSUPPORTED),
    "rescale": (dict(extra_flags=L.F_CFG_RESCALE), {}, L.ERR_UNSUPPORTED),
    "apg": (dict(extra_flags=L.F_CFG_APG), {}, L.ERR_UNSUPPORTED),
    "unipc": ({}, dict(form="UNIPC"), L.ERR_UNSUPPORTED),
    "stride": (dict(stride=2048 + 64), {}, L.ERR_UNSUPPORTED),
    "no_cfg": (dict(guidance=L.GUIDE["uncond"]), {}, L.ERR_ARG),
    "form": (dict(form_code=9), {}, L.ERR_ARG),
}


@gpu
@pytest.mark.parametrize("what", sorted(BAD))
def test_error_returns_write_nothing(what):
    kw, vkw, code = BAD[what]
    kw = dict(kw)
    guidance, form_code = kw.pop("guidance", None), kw.pop("form_code", None)
    v = dict(dict(form="LIN1", model="noise", tox0=True, store_m=True, dup=True, s=7.5), **vkw)
    dev = make_case(v, 2048, 3, torch.float16, torch.float16, seed=3, **kw).on(DEV)
    if guidance is not None:
        dev.st.guidance = guidance
    if form_code is not None:
        dev.st.form = form_code
    rc = launch(dev)
    assert rc == code, (rc, L.lib.dpm_last_error())
    assert b"DPM_F_CFG_ZSTAR" in L.lib.dpm_last_error() or what == "form"
    dev.verify(rc=rc)


@gpu
@pytest.mark.parametrize("table", [False, True])
def test_a_flagged_request_in_a_multi_request_call_runs_on_its_own(table):
    """three requests with per-request stages, the middle one flagged: its result is its own single launch's, the other two are
    what they are without it -- also in a table call (DPM_TABLE_FILL on the host, then DPM_TABLE_LAUNCH)"""
    sd = ed = torch.float16
    P, batch = 2048, 2
    plain = dict(form="TWO", model="noise", tox0=True, store_m=True, dup=True, s=7.5)
    cases = [make_case(dict(plain, form=f), P, batch, sd, ed, seed=21, req=r, per_request=True, flag=r == 1)
             for r, f in enumerate(("TWO", "MS3", "LIN1"))]
    wants = [run_double(c) for c in cases]
    single = run_case(make_case(dict(plain, form="MS3"), P, batch, sd, ed, seed=21, req=1, per_request=True))
    devs = [c.on(DEV) for c in cases]
    st = (L.Stage * 3)(*[d.st for d in devs])
    bs = (L.Buffers * 3)(*[d.b for d in devs])
    if table:
        nbytes = L.table_bytes(3)
        host = np.zeros(nbytes + 16, dtype=np.uint8)
        off = (-host.ctypes.data) % 16
        devs[0].opts.table_mode = L.TABLE_FILL
        bs[0].workspace = host.ctypes.data + off
        assert L.lib.dpm_stage_launch_multi(st, bs, 3, _stream()) == 0, L.lib.dpm_last_error()
        assert [int(w) for w in host[off:off + 16].view(np.uint32)][2:] == [3, 0]          # three requests, no run of rows
        tab = torch.from_numpy(host[off:off + nbytes].copy()).to(DEV)
        devs[0].opts.table_mode = L.TABLE_LAUNCH
        bs[0].workspace = tab.data_ptr()
    rc = L.lib.dpm_stage_launch_multi(st, bs, 3, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants)
    for name in ("x_out", "m_out", "x_out2"):
        assert torch.equal(devs[1].arenas[name].payload_bits(), single.arenas[name].payload_bits()), name
    # the two others without the flagged one next to them: the same bits
    pair_devs = [cases[r].on(DEV) for r in (0, 2)]
    pair_devs[0].opts.table_mode = 0
    st2, bs2 = (L.Stage * 2)(*[d.st for d in pair_devs]), (L.Buffers * 2)(*[d.b for d in pair_devs])
    assert L.lib.dpm_stage_launch_multi(st2, bs2, 2, _stream()) == 0, L.lib.dpm_last_error()
    torch.cuda.synchronize()
    for d, r in zip(pair_devs, (0, 2)):
        for name in ("x_out", "m_out", "x_out2"):
            assert torch.equal(d.arenas[name].payload_bits(), devs[r].arenas[name].payload_bits()), (r, name)


@gpu
def test_lockstep_multi_launches_flagged_requests_one_by_one():
    """dpm_stage_launch_multi with ONE stage record for three flagged requests: no fused variant, three launches, each
    request the bits of its double and of its lone launch"""
    sd, ed = torch.float32, torch.bfloat16
    v = dict(form="TWO", model="v", tox0=True, store_m=True, dup=True, s=1.5)
    cases = [make_case(v, 4100, 2, sd, ed, seed=33, req=r, outputs=correlated) for r in range(3)]
    for c in cases[1:]:
        C.memmove(C.byref(c.st), C.byref(cases[0].st), C.sizeof(L.Stage))
    wants, devs = [run_double(c) for c in cases], [c.on(DEV) for c in cases]
    bs = (L.Buffers * 3)(*[d.b for d in devs])
    rc = L.lib.dpm_stage_launch_multi(C.byref(devs[0].st), bs, 3, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants)
    for c, d in zip(cases, devs):
        lone = c.on(DEV)
        assert launch(lone) == 0
        for name in ("x_out", "m_out", "x_out2"):
            assert torch.equal(lone.arenas[name].payload_bits(), d.arenas[name].payload_bits()), name
