"""CFG-Zero* rows of the table-driven launch (DPM_TABLE_ZSTAR, stage_zstar_kernel_table) on the MI355X.  Kernel level, through
the C ABI and between guards (tests/guarded.py), with the cases of tests/test_gpu_cfg_zero_star.py: DPM_TABLE_FILL |
DPM_TABLE_ZSTAR into a host tensor, `copy_` to the device, DPM_TABLE_LAUNCH | DPM_TABLE_ZSTAR.  Every request must get the bits
of its own dpm_stage_launch AND of the numpy double (tests/zstar_double.py, whose inputs are checked decidable on the CPU first:
a does not depend on the summation order) -- there is no tolerance; the table and its guards must be intact; the launches are
counted by name.
The shapes are the smallest at which this kernel can go wrong: samples of 8 elements (one live lane), 4088 / 4096 / 4104 (around
one full iteration of 512 threads x 8), 16376 / 16384 (the last of the register path), 16392 (the first of the re-read path) and
32776 (a third re-read trip with a tail); groups of 1, 2 and 20 rows; 1, 2 and 3 samples per row, every sample with data of its
own; LIN1 / TWO / MS3 / DENOISE, STORE_M, the duplicate store and the guidance scale differ from row to row, model type and
DPM_F_TO_X0 from group to group.  All five dtype pairs at the sizes up to 4104, fp32/fp32 and fp16/fp16 beyond.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import guarded as G
from dpm_solver_amd import _lib as L
from test_gpu_cfg_zero_star import MODELS, PAIRS, PAIR_IDS, _Pristine, _bits, _values, correlated, make_case, run_double
from test_gpu_table import DEV, TableCall, _stream

gpu = pytest.mark.gpu
ZST = L.TABLE_ZSTAR
ALL6 = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_RESCALE | L.TABLE_APG | ZST
FORMS = ("LIN1", "TWO", "MS3", "DENOISE")
SCALES = (7.5, 1.5, 3.0)
SIZES = (8, 4088, 4096, 4104, 16376, 16384, 16392, 32776)
SMALL = SIZES[:4]                                   # ... where all five dtype pairs run; beyond: fp32/fp32 and fp16/fp16
# (rows, elements per sample, samples per row): every size with every group size, the samples per row in rotation
CELLS = [(rows, P, 1 + (i + k) % 3) for i, P in enumerate(SIZES) for k, rows in enumerate((1, 2, 20))]
CELL_IDS = ["%drow-per%d-b%d" % c for c in CELLS]
SWEEP = [(p, ci) for p in range(len(PAIRS)) for ci, c in enumerate(CELLS) if c[1] in SMALL or p in (0, 3)]
SWEEP_IDS = ["%s-%s" % (PAIR_IDS[p], CELL_IDS[ci]) for p, ci in SWEEP]


def seed_of(p, ci):
    return 7 * p + ci


def group_of(p, ci):
    """(model type, DPM_F_TO_X0) of dtype pair p at CELLS[ci]: what a group shares"""
    q = 3 * p + ci
    return MODELS[q % 4], (q // 4) % 2 == 0


def variant(q, model, tox0, forms=FORMS):
    """the record of row q of a call: form, STORE_M, the duplicate store and the scale all differ from row to row"""
    return dict(form=forms[q % len(forms)], model=model, tox0=tox0, store_m=q % 3 != 0, dup=q % 4 != 3, s=SCALES[(q // 2) % 3])


def requests(count, P, batch, sd, ed, model, tox0, seed=0, forms=FORMS, **kw):
    """the CPU cases of one per-request-stage call, every row with a record and data of its own; every other row draws
    o_c = 0.8 o_u + 0.6 z"""
    return [make_case(variant(r + seed, model, tox0, forms), P, batch, sd, ed, seed=seed, req=r, per_request=True,
                      outputs=correlated if (r + seed) % 2 else None, **kw) for r in range(count)]


def test_cells_cover_sizes_groups_batches_and_network_kinds():
    assert (PAIRS[0], PAIRS[3]) == ((torch.float32, torch.float32), (torch.float16, torch.float16)) and len(PAIRS) == 5
    assert {c[1] for c in CELLS} == set(SIZES) and len(CELLS) == 24
    for P in SIZES:
        assert {c[0] for c in CELLS if c[1] == P} == {1, 2, 20} and {c[2] for c in CELLS if c[1] == P} == {1, 2, 3}
        assert {p for p, ci in SWEEP if CELLS[ci][1] == P} == (set(range(5)) if P in SMALL else {0, 3})
    for count in (1, 2, 20):
        assert {c[2] for c in CELLS if c[0] == count} == {1, 2, 3}
    for p in (0, 3):
        assert {group_of(p, ci) for ci in range(len(CELLS))} == {(m, t) for m in MODELS for t in (True, False)}
    for p in range(5):
        met = {group_of(p, ci) for pp, ci in SWEEP if pp == p}
        assert {m for m, _ in met} == set(MODELS) and {t for _, t in met} == {True, False}
    rows = [variant(q, "noise", True) for q in range(20)]
    assert {v["form"] for v in rows} == set(FORMS) and {v["store_m"] for v in rows} == {True, False}
    assert {v["dup"] for v in rows} == {True, False} and {v["s"] for v in rows} == set(SCALES)


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_inputs_of_every_case_are_decidable(p):
    """the doubles of the whole sweep on the CPU: none of its samples has an a that depends on the summation order -- the
    precondition under which the GPU tests ask for equal bits (zstar_double.assert_inputs_decidable).  No case is dropped."""
    sd, ed = PAIRS[p]
    for pp, ci in SWEEP:
        if pp == p:
            count, P, batch = CELLS[ci]
            for c in requests(count, P, batch, sd, ed, *group_of(p, ci), seed=seed_of(p, ci)):
                run_double(c)


def mixed_cases(sdt):
    """20 CFG-Zero* + 20 plain requests of one call (the plain ones: the flag cleared)"""
    cases = requests(40, 4104, 1, sdt, sdt, "noise", True, seed=3, forms=("LIN1", "TWO", "MS3"))
    for c in cases[::2]:
        c.st.flags &= ~L.F_CFG_ZSTAR
    return cases


def disqualified_cases(sd, ed):
    """four rows of 8-element samples and, in the middle, a flagged request of 12-element samples"""
    cases = requests(4, 8, 3, sd, ed, "v", True, seed=11)
    cases.insert(2, requests(3, 12, 2, sd, ed, "v", True, seed=11)[2])
    return cases


def zero_sample_cases(sd, ed, P=4104):
    """three rows of three samples; sample 1 of row 1 has an all-zero unconditional output: a = 0, g = s * o_c there"""
    cases = requests(3, P, 3, sd, ed, "noise", False, seed=9)
    pr = dict(cases[1].pristine)
    e1 = _values(pr["e1"], ed).clone()
    e1[P:2 * P] = 0.0
    pr["e1"] = _bits(e1, ed)
    cases[1] = make_case(dict(variant(1 + 9, "noise", False), form="DENOISE", store_m=True, dup=True), P, 3, sd, ed, seed=9, req=1,
                         per_request=True, like=_Pristine(pr))
    return cases


def test_inputs_of_the_other_calls_are_decidable():
    """... and those of the calls outside the sweep that are compared with the double on the GPU"""
    import kernel_double as KD
    for sdt in (torch.float16, torch.float32):
        for c in mixed_cases(sdt):
            if c.st.flags & L.F_CFG_ZSTAR:
                run_double(c)
            else:
                G.run_double(c)
    for p in (0, 2, 4):
        for c in disqualified_cases(*PAIRS[p]) + zero_sample_cases(*PAIRS[p]):
            run_double(c)
    # the zero sample: the double itself stores s * o_c there (a DENOISE stage on the noise prediction stores g)
    c = zero_sample_cases(torch.float32, torch.float32)[1]
    run_double(c)
    P = 4104
    e0 = _values(c.pristine["e0"], torch.float32)[P:2 * P]
    want = _bits(torch.tensor(c.st.cfg_scale, dtype=torch.float32) * e0, torch.float32)
    assert torch.equal(c.arenas["x_out"].payload_bits()[P:2 * P], want)
    assert KD is not None


def names_of(fn):
    """names of the stage kernels fn() launches, one entry per launch (torch's profiler)"""
    from torch.profiler import ProfilerActivity, profile
    fn()                                                          # (first-launch costs outside the profile)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if "stage_" in e.key and "kernel" in e.key for _ in range(e.count)]


def _double(c):
    return run_double(c) if c.st.flags & L.F_CFG_ZSTAR else G.run_double(c)


def check_call(cases, what, check_own=True):
    """one FILL / copy / LAUNCH tick with the flag on guarded operands: guards, inputs and bits against the double (verify), the
    table and its guards as the host wrote them, then every request's own dpm_stage_launch into the same, refilled, output
    arenas: the same bits, guards included"""
    wants, devs = [_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = TableCall(devs, flags=ZST)
    assert t.host.numel() == L.table_bytes(len(cases))            # no section: the table of a call without the flag
    t.tick()
    G.verify_all(devs, wants)
    assert t.table_intact(), (what, "the kernel may only read its table")
    for r, d in enumerate(devs if check_own else ()):
        fused = {k: d.arenas[k].raw.clone() for k in G.OUTPUTS}
        for k in G.OUTPUTS:
            d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])
        rc = L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
        for k in G.OUTPUTS:
            assert torch.equal(fused[k], d.arenas[k].raw), (what, r, d.n, k, "differs from the request's own dpm_stage_launch")
    return t, devs, wants


@gpu
@pytest.mark.parametrize("p,ci", SWEEP, ids=SWEEP_IDS)
def test_zstar_table_calls_equal_the_single_launches_and_the_double(p, ci):
    sd, ed = PAIRS[p]
    count, P, batch = CELLS[ci]
    model, tox0 = group_of(p, ci)
    cases = requests(count, P, batch, sd, ed, model, tox0, seed=seed_of(p, ci))
    t, _, _ = check_call(cases, (model, tox0, count, P, batch))
    header = t.host[:16].view(torch.int32).tolist()
    assert header == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1], header


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_one_launch_per_group_counted_by_kernel_name(sdt):
    # a group of ONE, of 17 and of 40 CFG-Zero* rows, every form and scale among them: ONE stage_zstar_kernel_table launch
    for count in (1, 17, 40):
        t = TableCall([c.on(DEV) for c in requests(count, 4104, 1, sdt, sdt, "noise", True, seed=count)], flags=ZST)
        names = names_of(t.tick)
        assert len(names) == 1 and "stage_zstar_kernel_table" in names[0], (count, names)
    # 20 CFG-Zero* + 20 plain requests: two runs, one launch of either table family
    t, _, _ = check_call(mixed_cases(sdt), "CFG-Zero* beside plain", check_own=False)
    assert t.host[:16].view(torch.int32).tolist()[2:] == [40, 2]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_zstar_kernel_table" in n for n in names) == 1 and \
        sum("stage_kernel_table<" in n for n in names) == 1, names
    # without bit 4096 the same requests are launched one by one, as in version 216
    t = TableCall([c.on(DEV) for c in requests(5, 4104, 1, sdt, sdt, "noise", True, seed=5)], flags=ZST)
    names = names_of(lambda: t.tick(flags=0))
    assert len(names) == 5 and all("stage_zstar_kernel<" in n for n in names), names


@gpu
@pytest.mark.parametrize("p", [0, 2, 4], ids=[PAIR_IDS[i] for i in (0, 2, 4)])
def test_a_disqualified_row_takes_its_own_launch_in_the_same_call(p):
    """a flagged request of 12-element samples (no whole 8-element groups) among rows of the same n: no row -- its own
    stage_zstar_kernel launch in the same call, which still projects, beside the others' one table launch"""
    sd, ed = PAIRS[p]
    t, _, _ = check_call(disqualified_cases(sd, ed), "a sample of 12 elements")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [5, 1]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_zstar_kernel_table" in n for n in names) == 1 and \
        sum("stage_zstar_kernel<" in n for n in names) == 1, names


@gpu
@pytest.mark.parametrize("p", [0, 2, 4], ids=[PAIR_IDS[i] for i in (0, 2, 4)])
def test_a_zero_unconditional_sample_beside_ordinary_rows(p):
    """S_uu == 0 in one sample of one row: a = 0 there, g = s * o_c; that sample, the other samples of its row and the other
    rows of the same launch all keep the bits of the double and of the request's own launch"""
    sd, ed = PAIRS[p]
    t, devs, _ = check_call(zero_sample_cases(sd, ed), "a zero unconditional output")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [3, 1]
    if sd is torch.float32 and ed is torch.float32:                # the anchor that needs no double: a DENOISE stage stores g
        P, c = 4104, devs[1]
        e0 = _values(c.pristine["e0"], ed)[P:2 * P]
        want = _bits(torch.tensor(c.st.cfg_scale, dtype=torch.float32) * e0, sd)
        for name in ("x_out", "m_out", "x_out2"):
            assert torch.equal(c.arenas[name].payload_bits().cpu()[P:2 * P], want), name


@gpu
def test_all_six_flags_every_other_row_kind_beside_zstar_rows():
    """one call that carries all six table flags: the 29 requests of tests/test_gpu_table_kinds.py (plain / UniPC, MS3, SDE of
    two model types, thresholded of two ratios, mask-blend, ragged), two guidance-rescale rows, two APG rows (one with a
    momentum) and CFG-Zero* rows of two groups among them.  Every request the bits of its double; ONE table kernel per run, by
    name; the header counts the runs"""
    import apg_guarded as AG
    import test_gpu_table_apg as TA
    import test_gpu_table_kinds as TK
    import test_gpu_table_rescale as TR
    from test_gpu_edges import PAIRS as EPAIRS
    p, ci = 4, 0
    sd, ed = EPAIRS[p]
    kcases, kwants = TK.build(TK.KINDS, p, ci)
    rsc = TR.requests(2, 4104, 2, sd, ed, "noise", True, seed=2)
    apg = TA.requests(2, 4104, 1, sd, ed, "noise", seed=1)
    assert {c.st.thr_max != 0 for c in apg} == {True, False}
    za = requests(3, 4104, 2, sd, ed, "v", True, seed=4)
    zb = requests(2, 8, 3, sd, ed, "noise", False, seed=6)
    # in call order: request 0 plain (bs[0].workspace is the table), the per-sample kinds scattered among the 29
    order = ([("k", c, w) for c, w in zip(kcases, kwants)][:5] + [("z", za[0], None), ("r", rsc[0], None), ("a", apg[0], None)]
             + [("k", c, w) for c, w in zip(kcases, kwants)][5:20] + [("z", zb[0], None), ("z", za[1], None), ("a", apg[1], None)]
             + [("k", c, w) for c, w in zip(kcases, kwants)][20:] + [("r", rsc[1], None), ("z", zb[1], None), ("z", za[2], None)])
    wants, devs = [], []
    for kind, c, w in order:
        if kind == "k":
            wants.append(w)
        elif kind == "z":
            wants.append(run_double(c))
        elif kind == "r":
            wants.append(TR.run_double(c))
        else:
            wants.append(TA.run_double(c))
        if kind == "a":
            d = AG.on(c, DEV)
            d.b.thr_hint = d.avg.ptr
            devs.append(d)
        else:
            devs.append(c.on(DEV))
    t = TableCall(devs, flags=ALL6)
    assert t.host.numel() == L.table_bytes(len(devs), ALL6) == L.table_bytes(len(devs), ALL6 & ~ZST)
    t.tick()
    for (kind, _, _), d, w in zip(order, devs, wants):
        if kind == "a":
            AG.verify(d, w)
        else:
            d.verify(w)
    assert t.table_intact(), "the kernels may only read their table"
    kruns = TK.runs_of(TK.KINDS, TK.ALL)
    n_runs = len(kruns) + 1 + 1 + 2                                # + rescale, APG, two CFG-Zero* groups
    assert t.host[:16].view(torch.int32).tolist() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(devs), n_runs]
    names = names_of(t.tick)
    fam = lambda s: sum(s in n for n in names)
    assert fam("stage_zstar_kernel_table") == 2 and fam("stage_rescale_kernel_table") == 1 and fam("stage_apg_kernel_table") == 1
    for kind, family in TK.FAMILY.items():
        assert fam(family + "<") == sum(1 for k, _ in kruns if k == kind), (kind, names)
    n_fused, n_lone = TK.lone_launches(TK.KINDS, TK.ALL)
    assert len(names) == n_runs + n_fused + n_lone, names          # one kernel launch per run, the rest as mode 0 launches them
