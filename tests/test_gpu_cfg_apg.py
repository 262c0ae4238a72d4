"""The adaptive-projected-guidance stage kernel (DPM_F_CFG_APG, stage_apg_kernel) through the C ABI on guard-banded arenas
(tests/guarded.py, the fp32 running average in an arena of its own: tests/apg_guarded.py), bit for bit against its numpy double
(tests/apg_double.py, whose inputs are checked decidable on the CPU first: sc and q do not depend on the summation order).
Sample sizes sit on the kernel's own edges: 1 and 2 the smallest legal, 7 and 4100 ragged (one element per lane), 8 one group,
2048 a partial iteration, 16384 the last size whose c and d stay in registers, 16392 the first that reads its operands twice.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import apg_double as AD
import apg_guarded as AG
import guarded as G
import kernel_double as KD
from dpm_solver_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 2, 7, 8, 2048, 4100, 16384, 16392]
BATCHES = [1, 3]
OFFSET1 = [2048, 16392]                       # ... also one element past the 16-byte boundary: one element per lane, both paths
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
         (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)]
PAIR_IDS = ["%s-%s" % (G._name(s), G._name(e)) for s, e in PAIRS]
FORMS = {"LIN1": (L.FORM_LIN1, 0), "TWO": (L.FORM_TWO, 0), "TWO_BH": (L.FORM_TWO, L.F_BASE_HIST), "MS3": (L.FORM_MS3, 0),
         "SS3T": (L.FORM_SS3T, 0), "DENOISE": (L.FORM_DENOISE, 0)}
MODELS = ("noise", "v", "x_start", "score")
ETAS = (0.0, 0.5, 1.0)
# the norm threshold: off; far below the norm of any direction of these inputs (the cap active: |d| of one element of two
# normal outputs is below 1e-3 with probability 1e-3, of a larger sample never); far above any (the cap inactive)
RS = (0.0, 1e-3, 1e6)
BETAS = (0.0, -0.5)
PER_CELL = 3


def variants():
    """form x model type x momentum on / off, with STORE_M, x_out2, eta, r and the guidance scale in rotation: 48"""
    out = []
    for i, form in enumerate(FORMS):
        for j, model in enumerate(MODELS):
            for k, beta in enumerate(BETAS):
                q = 8 * i + 2 * j + k
                out.append(dict(form=form, model=model, beta=beta, store_m=(i + j + k) % 2 == 0, dup=(i + 2 * j + k) % 3 != 0,
                                eta=ETAS[q % 3], r=RS[(q // 3) % 3], s=(7.5, 1.5)[(q // 2) % 2]))
    return out


def plan(pair_index, batch):
    """[(P, offset, variant)] of one (dtype pair, batch): every size with PER_CELL variants in rotation, the offset cells too"""
    vs = variants()
    random.Random(31 * pair_index + batch).shuffle(vs)
    cells = [(P, 0) for P in SIZES] + [(P, 1) for P in OFFSET1]
    return [(P, off, vs[(PER_CELL * i + j) % len(vs)]) for i, (P, off) in enumerate(cells) for j in range(PER_CELL)]


def path_of(P, offset):
    return ("vec" if P % 8 == 0 and offset == 0 else "lane") + ("-keep" if P <= 16384 else "-reread")


def test_table_meets_the_coverage_rule():
    vs = variants()
    assert len(vs) == 48 and SIZES == [1, 2, 7, 8, 2048, 4100, 16384, 16392] and BATCHES == [1, 3] and len(set(PAIRS)) == 5
    assert {(v["eta"], v["r"], v["beta"]) for v in vs} == {(e, r, b) for e in ETAS for r in RS for b in BETAS}
    for key, vals in (("form", set(FORMS)), ("model", set(MODELS))):
        for val in vals:
            mine = [v for v in vs if v[key] == val]
            assert {v["beta"] for v in mine} == set(BETAS) and {v["store_m"] for v in mine} == {True, False}
            assert {v["dup"] for v in mine} == {True, False}
            assert {v["eta"] for v in mine} == set(ETAS) and {v["r"] for v in mine} == set(RS)
    met = {}
    for p in range(len(PAIRS)):
        for batch in BATCHES:
            pl = plan(p, batch)
            assert {(P, off) for P, off, _ in pl} == {(P, 0) for P in SIZES} | {(P, 1) for P in OFFSET1}
            for P, off, v in pl:
                met.setdefault(path_of(P, off), set()).update({v["form"], v["model"], ("pair", p), ("beta", v["beta"])})
    every = set(FORMS) | set(MODELS) | {("pair", p) for p in range(5)} | {("beta", b) for b in BETAS}
    assert set(met) == {"vec-keep", "lane-keep", "vec-reread", "lane-reread"}
    assert all(m == every for m in met.values()), {k: every - m for k, m in met.items()}


@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=PAIR_IDS)
def test_inputs_of_every_case_are_decidable(pair):
    """the doubles of the whole sweep on the CPU: none of its samples has an sc or a q that depends on the summation order
    (the precondition under which the GPU tests may ask for equal bits), and the double stays inside its payloads"""
    sd, ed = PAIRS[pair]
    for batch in BATCHES:
        for i, (P, off, v) in enumerate(plan(pair, batch)):
            run_double(make_case(v, P, batch, sd, ed, offset=off, seed=100 * pair + i))


def make_stage(v, seed=0, extra_flags=0):
    """a flagged stage record with scalars of realistic magnitude"""
    rng = random.Random(seed)
    st = L.Stage()
    form, fflags = FORMS[v["form"]] if v["form"] in FORMS else (L.FORM_UNIPC, 0)
    st.index, st.form, st.model_type, st.guidance = 3, form, L.MODEL[v["model"]], L.GUIDE["classifier-free"]
    st.flags = ((L.F_TO_X0 if v.get("tox0", True) else 0) | (L.F_STORE_M if v["store_m"] else 0) | fflags | L.F_CFG_APG
                | extra_flags)
    st.h1_slot = st.h2_slot = st.m_slot = -1
    a = rng.uniform(0.05, 0.999)
    st.alpha_e, st.sigma_e = a, math.sqrt(1.0 - a * a)
    st.cfg_scale, st.cg_scale, st.thr_ratio, st.thr_max = v["s"], v["eta"], v["r"], v["beta"]
    st.blend_alpha, st.blend_sigma = 0.8, 0.6
    st.cx, st.c0, st.c1, st.c2 = (rng.uniform(-2, 2) for _ in range(4))
    for j in range(4):
        st.k[j] = rng.uniform(-1.5, 1.5)
    st.k[4] = rng.uniform(0.5, 1.5)
    return st


def make_case(v, P, batch, sd, ed, offset=0, seed=0, req=0, like=None, per_request=False, avg_bits=None, **kw):
    """the guarded operands of one flagged launch; the running average: random values with a momentum (avg_bits: these
    instead), a poisoned arena without"""
    st = make_stage(v, seed * 131 + req, kw.pop("extra_flags", 0))
    case = G.GuardedLaunch("apg", st, P * batch, sd, ed, batch=batch, offset=offset, dup=v["dup"],
                           sep_xe=v["form"] in ("SS3T", "TWO_BH"), seed=seed, req=req, like=like,
                           per_request_stages=per_request, **kw)
    if avg_bits is None and v["beta"] != 0.0:
        avg_bits = AG.random_bits(P * batch, 1000 * seed + req)
    return AG.attach(case, avg_bits if v["beta"] != 0.0 else None)


def run_double(case):
    assert AD.launch_raw_double(KD._Ref(case.st), KD._Ref(case.b)) == 0      # (asserts the inputs decidable first)
    case.verify()
    case.avg.verify("average", case.avg.payload_bits() if case.st.thr_max != 0.0 else None)     # its guards; untouched without
    return case


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(dev):
    rc = L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), _stream())
    torch.cuda.synchronize()
    return rc


def run_case(case):
    want, dev = run_double(case), AG.on(case, DEV)
    rc = launch(dev)
    assert rc == 0, (rc, L.lib.dpm_last_error())
    AG.verify(dev, want)              # outputs and -- with a momentum -- the average: the double's bits, every guard intact;
    if "x_out2" in dev.written:       # without a momentum the poisoned workspace is untouched
        a, b = dev.arenas["x_out"], dev.arenas["x_out2"]
        assert torch.equal(a.payload_bits(), b.payload_bits())
    return dev


@gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=PAIR_IDS)
def test_sizes_forms_and_network_kinds(pair, batch):
    sd, ed = PAIRS[pair]
    for i, (P, off, v) in enumerate(plan(pair, batch)):
        try:
            run_case(make_case(v, P, batch, sd, ed, offset=off, seed=100 * pair + i))
        except AssertionError as e:
            raise AssertionError("P=%d batch=%d offset=%d %s: %s" % (P, batch, off, v, e)) from e


class _Pristine:
    def __init__(self, pristine):
        self.pristine = pristine


@gpu
@pytest.mark.parametrize("P", [7, 2048, 16392])
def test_a_sample_does_not_depend_on_the_batch_around_it(P):
    v = dict(form="TWO", model="v", beta=-0.5, store_m=True, dup=True, eta=0.5, r=1e-3, s=7.5)
    sd, ed = torch.float32, torch.float16
    whole_case = make_case(v, P, 3, sd, ed, seed=5)
    whole = run_case(whole_case)
    for k in range(3):
        one = _Pristine({name: bits[k * P:(k + 1) * P] for name, bits in whole.pristine.items()})
        alone = make_case(v, P, 1, sd, ed, seed=5, like=one, avg_bits=whole_case.avg_pristine[k * P:(k + 1) * P])
        assert bytes(alone.st) == bytes(whole.st)
        dev = run_case(alone)
        for name in ("x_out", "m_out", "x_out2"):
            assert torch.equal(dev.arenas[name].payload_bits().cpu(), whole.arenas[name].payload_bits().cpu()[k * P:(k + 1) * P]), (name, k)
        assert torch.equal(dev.avg.payload_bits().cpu(), whole.avg.payload_bits().cpu()[k * P:(k + 1) * P]), k


@gpu
@pytest.mark.parametrize("P,offset", [(2048, 0), (4100, 0), (16392, 0), (16392, 1)])
def test_the_average_holds_the_doubles_bits_and_a_poisoned_workspace_is_untouched(P, offset):
    """said outright (run_case holds every case of the sweep to it): after a launch with a momentum the average arena holds
    the double's new average between intact guards; without a momentum a workspace full of poison is neither read nor written"""
    sd, ed = torch.float16, torch.float16
    v = dict(form="MS3", model="noise", beta=-0.5, store_m=True, dup=False, eta=0.0, r=1e-3, s=7.5)
    case = make_case(v, P, 3, sd, ed, offset=offset, seed=41)
    before = case.avg_pristine.clone()
    dev = run_case(case)
    got = dev.avg.payload_bits().cpu()
    assert torch.equal(got, case.avg.payload_bits()) and not torch.equal(got, before)
    dev.avg.verify("average", got)                                            # (the guards)
    off = make_case(dict(v, beta=0.0), P, 3, sd, ed, offset=offset, seed=41)
    assert off.avg_pristine is None
    dev0 = run_case(off)
    dev0.avg.verify("poisoned workspace")                                     # as it was at construction: the fill pattern
    assert torch.equal(dev0.avg.payload_bits().cpu(), dev0.avg.before[dev0.avg.lead:dev0.avg.lead + dev0.avg.extent])


BAD = {
    "thresholding": (dict(extra_flags=L.F_THRESH), {}, L.ERR_UNSUPPORTED),
    "blend": (dict(extra_flags=L.F_BLEND, blend=(8, True)), {}, L.ERR_UNSUPPORTED),
    "noise": (dict(extra_flags=L.F_NOISE), {}, L.ERR_UNSUPPORTED),
    "rescale": (dict(extra_flags=L.F_CFG_RESCALE), {}, L.ERR_UNSUPPORTED),
    "unipc": ({}, dict(form="UNIPC"), L.ERR_UNSUPPORTED),
    "noise_prediction": ({}, dict(tox0=False), L.ERR_UNSUPPORTED),
    "stride": (dict(stride=4096), {}, L.ERR_UNSUPPORTED),
    "eta": ({}, dict(eta=1.5), L.ERR_ARG),
    "r": ({}, dict(r=-1.0), L.ERR_ARG),
    "beta": ({}, dict(beta=1.0), L.ERR_ARG),
    "no_average": (dict(null_ws=True), {}, L.ERR_ARG),
    "guidance": (dict(guidance=L.GUIDE["uncond"]), {}, L.ERR_ARG),
}


@gpu
@pytest.mark.parametrize("what", sorted(BAD))
def test_error_returns_write_nothing(what):
    kw, vkw, code = BAD[what]
    kw = dict(kw)
    null_ws, guidance = kw.pop("null_ws", False), kw.pop("guidance", None)
    v = dict(dict(form="LIN1", model="noise", beta=-0.5, store_m=True, dup=True, eta=0.5, r=1e-3, s=7.5), **vkw)
    case = make_case(v, 2048, 3, torch.float16, torch.float16, seed=3, **kw)
    if guidance is not None:
        case.st.guidance = guidance
    dev = AG.on(case, DEV)
    if null_ws:
        dev.b.workspace = None
    rc = launch(dev)
    assert rc == code, (rc, L.lib.dpm_last_error())
    AG.verify(dev, rc=rc)                                                     # no output byte, the running average neither


@gpu
@pytest.mark.parametrize("table", [False, True])
def test_a_flagged_request_in_a_multi_request_call_runs_on_its_own(table):
    """three requests with per-request stages, the middle one flagged (with a momentum): its result and its average are its own
    single launch's, the other two are what they are without it -- also in a table call (DPM_TABLE_FILL on the host, then
    DPM_TABLE_LAUNCH)"""
    sd = ed = torch.float16
    P, batch = 2048, 2
    flagged = dict(form="MS3", model="noise", beta=-0.5, store_m=True, dup=True, eta=0.5, r=1e-3, s=7.5)
    plain = dict(flagged, beta=0.0)
    cases = [make_case(dict(flagged if r == 1 else plain, form=f), P, batch, sd, ed, seed=21, req=r, per_request=True)
             for r, f in enumerate(("TWO", "MS3", "LIN1"))]
    for r in (0, 2):
        cases[r].st.flags &= ~L.F_CFG_APG
        cases[r].st.cg_scale, cases[r].st.thr_ratio, cases[r].st.thr_max = 4.5, 0.995, 1.0
        cases[r].b.workspace = None
    wants = [run_double(c) for c in cases]
    single = run_case(make_case(flagged, P, batch, sd, ed, seed=21, req=1, per_request=True))
    devs = [AG.on(c, DEV) for c in cases]
    for r in (0, 2):
        devs[r].b.workspace = None
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
    devs[1].avg.verify("average", wants[1].avg.payload_bits())
    for name in ("x_out", "m_out", "x_out2"):
        assert torch.equal(devs[1].arenas[name].payload_bits(), single.arenas[name].payload_bits()), name
    assert torch.equal(devs[1].avg.payload_bits(), single.avg.payload_bits())
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
    request the bits of its double and an average of its own"""
    sd, ed = torch.float32, torch.bfloat16
    v = dict(form="TWO", model="v", beta=-0.5, store_m=True, dup=True, eta=1.0, r=1e6, s=1.5)
    cases = [make_case(v, 4100, 2, sd, ed, seed=33, req=r) for r in range(3)]
    for c in cases[1:]:
        C.memmove(C.byref(c.st), C.byref(cases[0].st), C.sizeof(L.Stage))
    wants, devs = [run_double(c) for c in cases], [AG.on(c, DEV) for c in cases]
    bs = (L.Buffers * 3)(*[d.b for d in devs])
    rc = L.lib.dpm_stage_launch_multi(C.byref(devs[0].st), bs, 3, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    for d, w in zip(devs, wants):
        AG.verify(d, w)
