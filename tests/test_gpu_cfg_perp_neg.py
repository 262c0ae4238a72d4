"""The Perp-Neg stage kernel (DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 record, stage_perp_kernel) through the C ABI on guard-banded
arenas (tests/guarded.py, tests/pair_guarded.py, tests/perp_guarded.py), bit for bit against its numpy double
(tests/perp_double.py, whose inputs are checked decidable on the CPU first: a does not depend on the summation order).  Sample
sizes sit on the kernel's own edges: 1 the smallest legal, 7 and 4100 ragged (one element per lane), 8 one group, 2048 a partial
iteration, 16384 the last size of the register / LDS path, 16392 the first that reads its three outputs twice.  Half of the cases
draw three independent normal outputs (the two differences share o_u, so a is near 0.5), half o_n = o_u + 0.8 (o_c - o_u) + 0.6 z
(a near 0.8).  Three anchors need no
double: g == e0, g == e1 and e0 == e1.  No case is skipped or reseeded at run time: the seeds are the ones below.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import guarded as G
import kernel_double as KD
import perp_double as PP
import perp_guarded as PG
from dpm_solver_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
PAIR, CFG = L.GUIDE["classifier-free-2"], L.GUIDE["classifier-free"]
SIZES = [1, 7, 8, 2048, 4100, 16384, 16392]
BATCHES = [1, 3]
OFFSET1 = [2048, 16392]                       # ... also one element past the 16-byte boundary: one element per lane, both paths
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
         (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)]
PAIR_IDS = ["%s-%s" % (G._name(s), G._name(e)) for s, e in PAIRS]
FORMS = {"LIN1": (L.FORM_LIN1, 0), "TWO": (L.FORM_TWO, 0), "TWO_BH": (L.FORM_TWO, L.F_BASE_HIST), "MS3": (L.FORM_MS3, 0),
         "SS3T": (L.FORM_SS3T, 0), "DENOISE": (L.FORM_DENOISE, 0)}
MODELS = ("noise", "v", "x_start", "score")
SCALES = ((7.5, 1.0), (3.0, 2.5))             # (s, w): the guidance and the negative scale
PER_CELL = 3


def variants():
    """form x model type x DPM_F_TO_X0, with STORE_M and (s, w) in rotation: 48"""
    out = []
    for i, form in enumerate(FORMS):
        for j, model in enumerate(MODELS):
            for k, tox0 in enumerate((True, False)):
                out.append(dict(form=form, model=model, tox0=tox0, store_m=(i + j + k) % 2 == 0, sw=SCALES[(i + j // 2 + k) % 2]))
    return out


def plan(pair_index, batch):
    """[(P, offset, variant)] of one (dtype pair, batch): every size with PER_CELL variants in rotation, the offset cells too"""
    vs = variants()
    random.Random(41 * pair_index + batch).shuffle(vs)
    cells = [(P, 0) for P in SIZES] + [(P, 1) for P in OFFSET1]
    return [(P, off, vs[(PER_CELL * i + j) % len(vs)]) for i, (P, off) in enumerate(cells) for j in range(PER_CELL)]


def path_of(P, offset):
    return ("vec" if P % 8 == 0 and offset == 0 else "lane") + ("-keep" if P <= 16384 else "-reread")


def test_table_meets_the_coverage_rule():
    vs = variants()
    assert len(vs) == 48 and SIZES == [1, 7, 8, 2048, 4100, 16384, 16392] and BATCHES == [1, 3] and len(set(PAIRS)) == 5
    assert OFFSET1 == [2048, 16392]
    for key, vals in (("form", set(FORMS)), ("model", set(MODELS))):
        for val in vals:
            mine = [v for v in vs if v[key] == val]
            assert {v["tox0"] for v in mine} == {True, False} and {v["store_m"] for v in mine} == {True, False}
            assert {v["sw"] for v in mine} == set(SCALES)
    met, mix = {}, {}
    for p in range(len(PAIRS)):
        for batch in BATCHES:
            pl = plan(p, batch)
            assert {(P, off) for P, off, _ in pl} == {(P, 0) for P in SIZES} | {(P, 1) for P in OFFSET1}
            for i, (P, off, v) in enumerate(pl):
                met.setdefault(path_of(P, off), set()).update({v["form"], v["model"], ("pair", p), ("tox0", v["tox0"])})
                mix.setdefault((P, off), set()).add(i % 2)
    every = set(FORMS) | set(MODELS) | {("pair", p) for p in range(5)} | {("tox0", True), ("tox0", False)}
    assert set(met) == {"vec-keep", "lane-keep", "vec-reread", "lane-reread"}
    assert all(m == every for m in met.values()), {k: every - m for k, m in met.items()}
    assert all(m == {0, 1} for m in mix.values())              # every cell meets both input mixes


def make_stage(v, seed=0, extra_flags=0, flag=True):
    """a flagged stage record with scalars of realistic magnitude"""
    rng = random.Random(seed)
    st = L.Stage()
    form, fflags = FORMS[v["form"]] if v["form"] in FORMS else (L.FORM_UNIPC, 0)
    st.index, st.form, st.model_type, st.guidance = 3, form, L.MODEL[v["model"]], PAIR
    st.flags = ((L.F_TO_X0 if v["tox0"] else 0) | (L.F_STORE_M if v["store_m"] else 0) | fflags
                | (L.F_CFG2_PERP if flag else 0) | extra_flags)
    st.h1_slot = st.h2_slot = st.m_slot = -1
    a = rng.uniform(0.05, 0.999)
    st.alpha_e, st.sigma_e = a, math.sqrt(1.0 - a * a)
    st.cfg_scale, st.cg_scale = v["sw"]
    st.thr_ratio, st.thr_max = 0.995, 1.0
    st.blend_alpha, st.blend_sigma = 0.8, 0.6
    st.cx, st.c0, st.c1, st.c2 = (rng.uniform(-2, 2) for _ in range(4))
    for j in range(4):
        st.k[j] = rng.uniform(-1.5, 1.5)
    st.k[4] = rng.uniform(0.5, 1.5)
    return st


def make_case(v, P, batch, sd, ed, offset=0, seed=0, req=0, like=None, per_request=False, outputs=None, flag=True, **kw):
    st = make_stage(v, seed * 131 + req, kw.pop("extra_flags", 0), flag)
    return PG.make_case(st, P * batch, batch, sd, ed, outputs=outputs, like=like, offset=offset,
                        sep_xe=v["form"] in ("SS3T", "TWO_BH"), seed=seed, req=req, per_request_stages=per_request, **kw)


def correlated(e0, e1, z):
    """o_n = o_u + 0.8 (o_c - o_u) + 0.6 z: the negative direction leans on the positive one, a near 0.8"""
    return e0, e1, e1 + 0.8 * (e0 - e1) + 0.6 * z


def sweep_case(pair, batch, i, P, off, v):
    sd, ed = PAIRS[pair]
    return make_case(v, P, batch, sd, ed, offset=off, seed=100 * pair + i, outputs=correlated if i % 2 else None)


@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=PAIR_IDS)
def test_inputs_of_every_case_are_decidable(pair):
    """the doubles of the whole sweep on the CPU: none of its samples has an a that depends on the summation order (the
    precondition under which the GPU tests may ask for equal bits), and the double stays inside its payloads.  The correlated
    cases do land near 0.8 and the independent ones near 0.5 (d0 and d2 share o_u: <d2, d0> / <d0, d0> -> 1 / 2) wherever a sample
    is large enough to say so."""
    for batch in BATCHES:
        for i, (P, off, v) in enumerate(plan(pair, batch)):
            case = PG.run_double(sweep_case(pair, batch, i, P, off, v))
            if P >= 2048:
                ed = PAIRS[pair][1]
                a = PP.projection(*(PG.values(case.pristine[k], ed).numpy().reshape(batch, P) for k in ("e0", "e1", "g")))
                assert np.all(np.abs(a - (0.8 if i % 2 else 0.5)) < 0.1), (P, i, a)


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


@gpu
@pytest.mark.parametrize("P", [7, 2048, 16392])
def test_a_sample_does_not_depend_on_the_batch_around_it(P):
    v = dict(form="TWO", model="v", tox0=True, store_m=True, sw=(7.5, 1.0))
    sd, ed = torch.float32, torch.float16
    whole = run_case(make_case(v, P, 3, sd, ed, seed=5, outputs=correlated))
    for k in range(3):
        one = PG._Pristine({name: b[k * P:(k + 1) * P] for name, b in whole.pristine.items()})
        alone = make_case(v, P, 1, sd, ed, seed=5, like=one)
        assert bytes(alone.st) == bytes(whole.st)
        dev = run_case(alone)
        for name in ("x_out", "m_out"):
            assert torch.equal(dev.arenas[name].payload_bits().cpu(), whole.arenas[name].payload_bits().cpu()[k * P:(k + 1) * P]), (name, k)


# ------------------------------------------------------------------------------------------------
# the three anchors of the contract: an fp32 noise network, DPM_F_TO_X0 off, a DENOISE stage stores gd itself.  Each is held
# against a torch fp32 expression that needs no projection, against the double, and against the same record under another w
# where the identity says w does not matter.
# ------------------------------------------------------------------------------------------------
def _gpu_bits(case, want=None):
    dev = case.on(DEV)
    rc = launch(dev)
    assert rc == 0, (rc, L.lib.dpm_last_error())
    dev.verify(want)
    return {name: dev.arenas[name].payload_bits().cpu() for name in dev.written}


ANCHOR_SIZES = [(7, 3), (2048, 3), (16384, 2), (16392, 2)]
ANCHOR = dict(form="DENOISE", model="noise", tox0=False, store_m=True)
F = torch.float32


def _cfg_blend(case, s):
    e0, e1 = (PG.values(case.pristine[k], F) for k in ("e0", "e1"))
    return PG.bits(e1 + torch.tensor(s, dtype=F) * (e0 - e1), F)              # o_u + s * d0, one rounding per operation


@gpu
@pytest.mark.parametrize("same", ["e0", "e1"])
@pytest.mark.parametrize("P,batch", ANCHOR_SIZES)
def test_a_negative_equal_to_the_positive_or_to_the_unconditional_output_is_plain_guidance(P, batch, same):
    """g == e0: d2 == d0, a = 1, perp = 0; g == e1: d2 = 0, a = 0, perp = 0.  Either way gd = o_u + s * d0 whatever w."""
    pick = (lambda e0, e1, g: (e0, e1, e0.clone())) if same == "e0" else (lambda e0, e1, g: (e0, e1, e1.clone()))
    got = []
    for w in (1.0, 2.5, -0.75):
        case = make_case(dict(ANCHOR, sw=(7.5, w)), P, batch, F, F, seed=43, outputs=pick)
        got.append(_gpu_bits(case, PG.run_double(case)))
        for name in ("x_out", "m_out"):
            assert torch.equal(got[-1][name], _cfg_blend(case, 7.5)), (name, w)
    # ... and with the record's g pointing AT the other operand's arena (one buffer read as two operands)
    case = make_case(dict(ANCHOR, sw=(7.5, 2.5)), P, batch, F, F, seed=43)
    dev = case.on(DEV).share("g", same)
    assert launch(dev) == 0, L.lib.dpm_last_error()
    dev.verify()
    assert torch.equal(dev.arenas["x_out"].payload_bits().cpu(), _cfg_blend(case, 7.5))


@gpu
@pytest.mark.parametrize("P,batch", ANCHOR_SIZES)
def test_equal_positive_and_unconditional_outputs_subtract_the_whole_negative_direction(P, batch):
    """e0 == e1: d0 = 0, S_dd = 0, a = 0 (defined, no division) and gd = o_u + s * (0 - w * d2)"""
    for w in (1.0, 2.5):
        case = make_case(dict(ANCHOR, sw=(3.0, w)), P, batch, F, F, seed=47, outputs=lambda e0, e1, g: (e1.clone(), e1, g))
        got = _gpu_bits(case, PG.run_double(case))
        e1, g = (PG.values(case.pristine[k], F) for k in ("e1", "g"))
        want = PG.bits(e1 + torch.tensor(3.0, dtype=F) * (torch.zeros_like(e1) - torch.tensor(w, dtype=F) * (g - e1)), F)
        for name in ("x_out", "m_out"):
            assert torch.equal(got[name], want), (name, w)


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
    "rescale": (dict(extra_flags=L.F_CFG_RESCALE), {}, L.ERR_ARG),
    "zstar": (dict(extra_flags=L.F_CFG_ZSTAR), {}, L.ERR_ARG),
    "cfg": (dict(guidance=CFG), {}, L.ERR_ARG),
    "uncond": (dict(guidance=L.GUIDE["uncond"]), {}, L.ERR_ARG),
    "form": (dict(form_code=9), {}, L.ERR_ARG),
    "w_nan": (dict(w=float("nan")), {}, L.ERR_ARG),
    "s_inf": (dict(s=float("inf")), {}, L.ERR_ARG),
    "no_g": (dict(without=("g",)), {}, L.ERR_ARG),
    "no_e1": (dict(without=("e1",)), {}, L.ERR_ARG),
}


@gpu
@pytest.mark.parametrize("what", sorted(BAD))
def test_error_returns_write_nothing(what):
    kw, vkw, code = BAD[what]
    kw = dict(kw)
    guidance, form_code, stride = kw.pop("guidance", None), kw.pop("form_code", None), kw.pop("eps_stride", None)
    s, w = kw.pop("s", None), kw.pop("w", None)
    v = dict(dict(form="LIN1", model="noise", tox0=True, store_m=True, sw=(7.5, 1.0)), **vkw)
    dev = make_case(v, 2048, 3, torch.float16, torch.float16, seed=3, **kw).on(DEV)
    if guidance is not None:
        dev.st.guidance = guidance
    if form_code is not None:
        dev.st.form = form_code
    if stride is not None:
        dev.b.eps_stride = stride
    if s is not None:
        dev.st.cfg_scale = s
    if w is not None:
        dev.st.cg_scale = w
    rc = launch(dev)
    assert rc == code, (rc, L.lib.dpm_last_error())
    dev.verify(rc=rc)


@gpu
@pytest.mark.parametrize("mode", [L.TABLE_FILL, L.TABLE_LAUNCH | L.TABLE_PAIR])
def test_a_table_mode_call_with_a_flagged_request_writes_nothing(mode):
    sd = ed = torch.float16
    v = dict(form="TWO", model="noise", tox0=True, store_m=True, sw=(7.5, 1.0))
    devs = [make_case(v, 2048, 2, sd, ed, seed=23, req=r, per_request=True, flag=r == 1).on(DEV) for r in range(2)]
    st, bs = (L.Stage * 2)(*[d.st for d in devs]), (L.Buffers * 2)(*[d.b for d in devs])
    table = torch.zeros(L.table_bytes(2, mode & L.TABLE_PAIR) + 16, dtype=torch.uint8, device=DEV if mode & L.TABLE_LAUNCH else "cpu")
    devs[0].opts.table_mode = mode
    bs[0].workspace = table.data_ptr() + (-table.data_ptr()) % 16
    rc = L.lib.dpm_stage_launch_multi(st, bs, 2, _stream())
    torch.cuda.synchronize()
    assert rc == L.ERR_UNSUPPORTED and b"DPM_F_CFG2_PERP in a table-mode call" in L.lib.dpm_last_error()
    G.verify_all(devs, rc=rc)
    assert not bool(table.any())


def _plain_case(form, P, batch, sd, ed, seed, req):
    """a classifier-free request without any of this: guarded.GuardedLaunch's own operands"""
    v = dict(form=form, model="noise", tox0=True, store_m=True, sw=(7.5, 1.0))
    st = make_stage(v, seed * 131 + req, flag=False)
    st.guidance, st.cg_scale = CFG, 7.5 * st.sigma_e
    return G.GuardedLaunch("plain", st, P * batch, sd, ed, batch=batch, seed=seed, req=req, per_request_stages=True)


def _plain_double(case):
    assert PP.launch_raw_double(KD._Ref(case.st), KD._Ref(case.b), None) == 0
    case.verify()
    return case


@gpu
def test_a_flagged_request_in_a_multi_request_call_runs_on_its_own():
    """three requests with per-request stages, the middle one flagged: its result is its own single launch's, the other two are
    what they are without it"""
    sd = ed = torch.float16
    P, batch = 2048, 2
    flagged = make_case(dict(form="MS3", model="noise", tox0=True, store_m=True, sw=(7.5, 1.0)), P, batch, sd, ed, seed=21, req=1,
                        per_request=True, outputs=correlated)
    cases = [_plain_case("TWO", P, batch, sd, ed, 21, 0), flagged, _plain_case("LIN1", P, batch, sd, ed, 21, 2)]
    wants = [_plain_double(cases[0]), PG.run_double(cases[1]), _plain_double(cases[2])]
    single = run_case(flagged)
    devs = [c.on(DEV) for c in cases]
    st = (L.Stage * 3)(*[d.st for d in devs])
    bs = (L.Buffers * 3)(*[d.b for d in devs])
    rc = L.lib.dpm_stage_launch_multi(st, bs, 3, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants)
    for name in ("x_out", "m_out"):
        assert torch.equal(devs[1].arenas[name].payload_bits(), single.arenas[name].payload_bits()), name
    # the two others without the flagged one next to them: the same bits
    two = [cases[r].on(DEV) for r in (0, 2)]
    st2, bs2 = (L.Stage * 2)(*[d.st for d in two]), (L.Buffers * 2)(*[d.b for d in two])
    assert L.lib.dpm_stage_launch_multi(st2, bs2, 2, _stream()) == 0, L.lib.dpm_last_error()
    torch.cuda.synchronize()
    for d, r in zip(two, (0, 2)):
        for name in ("x_out", "m_out"):
            assert torch.equal(d.arenas[name].payload_bits(), devs[r].arenas[name].payload_bits()), (r, name)


@gpu
def test_lockstep_multi_launches_flagged_requests_one_by_one():
    """dpm_stage_launch_multi with ONE stage record for three flagged requests: no fused variant, three launches, each
    request the bits of its double and of its lone launch"""
    sd, ed = torch.float32, torch.bfloat16
    v = dict(form="TWO", model="v", tox0=True, store_m=True, sw=(3.0, 2.5))
    cases = [make_case(v, 4100, 2, sd, ed, seed=33, req=r, outputs=correlated) for r in range(3)]
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
