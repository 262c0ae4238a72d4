"""Perp-Neg rows of the table-driven launch (DPM_TABLE_PERP, stage_perp_kernel_table) on the MI355X.  Kernel level, through the
C ABI and between guards (tests/pair_guarded.py, tests/test_gpu_table_pair.py's PairRow): DPM_TABLE_FILL | DPM_TABLE_PERP into a
host tensor, `copy_` to the device, DPM_TABLE_LAUNCH | DPM_TABLE_PERP.  Every request must get the bits of its own
dpm_stage_launch (mode 0, no copies) AND of the numpy double (tests/table_perp_double.py, whose inputs are checked decidable on the
CPU first: a does not depend on the summation order) -- there is no tolerance; both copies must equal x_out; every guard band, the
third copy's and the table's included, must be intact, and so must the third copy's arena on rows without copies; the launches
are counted by name.
The shapes are the smallest at which this kernel can go wrong: samples of 8 elements (one live lane), 4088 / 4096 / 4104 (around
one full iteration of 512 threads x 8), 16376 / 16384 (the last of the register path), 16392 (the first of the re-read path) and
32776 (a third re-read trip with a tail); groups of 1, 2 and 20 rows; 1, 2 and 3 samples per row, every sample with data of its
own; LIN1 / TWO / MS3 / DENOISE, STORE_M, the copies and both scales differ from row to row, model type and DPM_F_TO_X0 from
group to group.  All five dtype pairs at the sizes up to 4104, fp32/fp32 and fp16/fp16 beyond.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import guarded as G
import kernel_double as KD
import perp_guarded as PG
import table_perp_double as TPP
from dpm_solver_amd import _lib as L
from test_gpu_cfg_perp_neg import MODELS, PAIR_IDS, PAIRS, correlated, make_stage
from test_gpu_table_pair import PairRow

gpu = pytest.mark.gpu
DEV = "cuda:0"
PP, PR = L.TABLE_PERP, L.TABLE_PAIR
ALL8 = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_RESCALE | L.TABLE_APG | L.TABLE_ZSTAR | PR | PP
FORMS = ("LIN1", "TWO", "MS3", "DENOISE")
SW = ((7.5, 1.0), (3.0, 2.5), (1.5, -0.75))         # (s, w): the guidance and the negative scale
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
    """the record of row q of a call: form, STORE_M, the copies and both scales all differ from row to row"""
    return dict(form=forms[q % len(forms)], model=model, tox0=tox0, store_m=q % 3 != 0, copies=q % 4 != 3, sw=SW[(q // 2) % 3])


class PerpRow(PairRow):
    """test_gpu_table_pair.PairRow under DPM_F_CFG2_PERP: the same operands and the same two copies"""

    def on(self, device, copies=None):
        kw = dict(self.kw)
        kw.pop("dup")
        return PerpRow(self.st, self.n, self.sd, self.ed, copies=self.copies if copies is None else copies, device=device,
                       like=self, **kw)


def make_row(v, P, batch, sd, ed, seed=0, req=0, outputs=None, stage_seed=None):
    """one CPU case; outputs: None -- three independent normal outputs; else f(e0, e1, g) -> (e0, e1, g) on the drawn values"""
    st = make_stage(v, seed * 131 + req if stage_seed is None else stage_seed)
    mk = lambda like: PerpRow(st, P * batch, sd, ed, copies=v["copies"], like=like, batch=batch, seed=seed, req=req,
                              per_request_stages=True)
    case = mk(None)
    if outputs is None:
        return case
    pr = dict(case.pristine)
    e0, e1, g = outputs(*(PG.values(pr[k], ed) for k in ("e0", "e1", "g")))
    pr["e0"], pr["e1"], pr["g"] = PG.bits(e0, ed), PG.bits(e1, ed), PG.bits(g, ed)
    return mk(PG._Pristine(pr))


def requests(count, P, batch, sd, ed, model, tox0, seed=0, forms=FORMS):
    """the CPU cases of one per-request-stage call, every row with a record and data of its own; every other row draws
    o_n = o_u + 0.8 (o_c - o_u) + 0.6 z"""
    return [make_row(variant(r + seed, model, tox0, forms), P, batch, sd, ed, seed=seed, req=r,
                     outputs=correlated if (r + seed) % 2 else None) for r in range(count)]


def run_double(case):
    """the table call's double on one CPU case -- its inputs asserted decidable first --: the stage, then the copies"""
    assert TPP.row_stage(case.st, case.b) == 0
    case.verify()
    return case


def test_cells_cover_sizes_groups_batches_and_network_kinds():
    assert (PAIRS[0], PAIRS[3]) == ((torch.float32, torch.float32), (torch.float16, torch.float16)) and len(PAIRS) == 5
    assert {c[1] for c in CELLS} == set(SIZES) and len(CELLS) == 24
    for P in SIZES:
        assert {c[0] for c in CELLS if c[1] == P} == {1, 2, 20} and {c[2] for c in CELLS if c[1] == P} == {1, 2, 3}
        assert {p for p, ci in SWEEP if CELLS[ci][1] == P} == (set(range(5)) if P in SMALL else {0, 3})
    for p in (0, 3):
        assert {group_of(p, ci) for ci in range(len(CELLS))} == {(m, t) for m in MODELS for t in (True, False)}
    for p in range(5):
        met = {group_of(p, ci) for pp, ci in SWEEP if pp == p}
        assert {m for m, _ in met} == set(MODELS) and {t for _, t in met} == {True, False}
    rows = [variant(q, "noise", True) for q in range(20)]
    assert {v["form"] for v in rows} == set(FORMS) and {v["store_m"] for v in rows} == {True, False}
    assert {v["copies"] for v in rows} == {True, False} and {v["sw"] for v in rows} == set(SW)


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_inputs_of_every_case_are_decidable(p):
    """the doubles of the whole sweep on the CPU: none of its samples has an a that depends on the summation order -- the
    precondition under which the GPU tests ask for equal bits (perp_double.assert_inputs_decidable).  No case is dropped."""
    sd, ed = PAIRS[p]
    for pp, ci in SWEEP:
        if pp == p:
            count, P, batch = CELLS[ci]
            for c in requests(count, P, batch, sd, ed, *group_of(p, ci), seed=seed_of(p, ci)):
                run_double(c)


def disqualified_cases(sd, ed):
    """four rows of 8-element samples and, in the middle, a flagged request of 12-element samples without copies"""
    cases = requests(4, 8, 3, sd, ed, "v", True, seed=11)
    cases.insert(2, make_row(dict(variant(2 + 11, "v", True), copies=False), 12, 2, sd, ed, seed=11, req=2, outputs=correlated))
    return cases


ANCHOR = dict(form="DENOISE", model="noise", tox0=False, store_m=True, copies=True)


def anchor_cases(sd, ed, P=4104):
    """three rows of three samples beside each other in ONE launch: row 0 ordinary; row 1 a negative equal to the positive
    (d2 = d0, a = 1, perp = 0: plain guidance whatever w); row 2 with o_c == o_u in its sample 1 (d0 = 0, S_dd = 0, a = 0 there:
    gd = o_u - s * w * d2), its other samples ordinary"""
    def zero_d0(e0, e1, g):
        e0 = e0.clone()
        e0[P:2 * P] = e1[P:2 * P]
        return e0, e1, g
    return [make_row(variant(9, "noise", False), P, 3, sd, ed, seed=9, req=0, outputs=correlated),
            make_row(dict(ANCHOR, sw=(7.5, 2.5)), P, 3, sd, ed, seed=9, req=1, outputs=lambda e0, e1, g: (e0, e1, e0.clone())),
            make_row(dict(ANCHOR, sw=(3.0, 2.5)), P, 3, sd, ed, seed=9, req=2, outputs=zero_d0)]


def test_inputs_of_the_other_calls_are_decidable():
    """... and those of the calls outside the sweep that are compared with the double on the GPU"""
    for p in (0, 2, 4):
        for c in disqualified_cases(*PAIRS[p]) + anchor_cases(*PAIRS[p]):
            run_double(c)
    for sdt in (torch.float16, torch.float32):
        for count in (1, 17, 40):
            for c in requests(count, 4104, 1, sdt, sdt, "noise", True, seed=count):
                run_double(c)
    sd, ed = PAIRS[4]
    for c in requests(3, 4104, 2, sd, ed, "v", True, seed=4) + requests(2, 8, 3, sd, ed, "noise", False, seed=6):
        run_double(c)
    # the anchors on the double itself (fp32, a DENOISE stage on the noise prediction stores gd)
    F = torch.float32
    P = 4104
    _, same, zero = [run_double(c) for c in anchor_cases(F, F)]
    e0, e1 = (PG.values(same.pristine[k], F) for k in ("e0", "e1"))
    assert torch.equal(same.arenas["x_out"].payload_bits(), PG.bits(e1 + torch.tensor(7.5, dtype=F) * (e0 - e1), F))
    e1, g = (PG.values(zero.pristine[k], F)[P:2 * P] for k in ("e1", "g"))
    want = PG.bits(e1 + torch.tensor(3.0, dtype=F) * (torch.zeros_like(e1) - torch.tensor(2.5, dtype=F) * (g - e1)), F)
    assert torch.equal(zero.arenas["x_out"].payload_bits()[P:2 * P], want)
    assert KD is not None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_call(cases, what, flags=PP):
    """one FILL / copy / LAUNCH tick with the flag on guarded operands: guards, inputs, bits against the double and the copies
    (verify: on a row without copies the third copy's arena must be untouched), the table and its guards as the host wrote them,
    then every request's own dpm_stage_launch -- mode 0, no copies -- on the same inputs: the same bits in x_out and m_out"""
    from test_gpu_table import TableCall
    wants, devs = [run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = TableCall(devs, flags=flags)
    assert t.host.numel() == L.table_bytes(len(cases), flags) == L.table_bytes(len(cases), flags | PR)
    t.tick()
    G.verify_all(devs, wants)
    assert t.table_intact(), (what, "the kernel may only read its table")
    for r, (c, d) in enumerate(zip(cases, devs)):
        lone = c.on(DEV, copies=False)
        rc = L.lib.dpm_stage_launch(C.byref(lone.st), C.byref(lone.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
        lone.verify()
        for k in ("x_out", "m_out"):
            assert torch.equal(lone.arenas[k].payload_bits(), d.arenas[k].payload_bits()), (
                what, r, d.n, k, "differs from the request's own dpm_stage_launch")
    return t, devs


@gpu
@pytest.mark.parametrize("p,ci", SWEEP, ids=SWEEP_IDS)
def test_perp_table_calls_equal_the_single_launches_and_the_double(p, ci):
    sd, ed = PAIRS[p]
    count, P, batch = CELLS[ci]
    model, tox0 = group_of(p, ci)
    cases = requests(count, P, batch, sd, ed, model, tox0, seed=seed_of(p, ci))
    t, _ = check_call(cases, (model, tox0, count, P, batch))
    header = t.host[:16].view(torch.int32).tolist()
    assert header == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1], header


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_one_launch_per_group_counted_by_kernel_name(sdt):
    from test_gpu_table import TableCall
    from test_gpu_table_zstar import names_of
    # a group of ONE, of 17 and of 40 Perp-Neg rows, every form, both kinds of row and every scale among them: ONE launch of
    # stage_perp_kernel_table, never a lone stage_perp_kernel for a row
    for count in (1, 17, 40):
        t = TableCall([c.on(DEV) for c in requests(count, 4104, 1, sdt, sdt, "noise", True, seed=count)], flags=PP)
        names = names_of(t.tick)
        assert len(names) == 1 and "stage_perp_kernel_table" in names[0], (count, names)
    # two groups (model type): two launches
    cases = requests(6, 4104, 2, sdt, sdt, "noise", True, seed=2) + requests(5, 4104, 2, sdt, sdt, "v", True, seed=3)
    t, _ = check_call(cases, "two groups")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [11, 2]
    names = names_of(t.tick)
    assert len(names) == 2 and all("stage_perp_kernel_table" in n for n in names), names


@gpu
@pytest.mark.parametrize("flags", [PP, PP | PR], ids=["perp", "perp+pair"])
@pytest.mark.parametrize("p", [0, 2, 4], ids=[PAIR_IDS[i] for i in (0, 2, 4)])
def test_a_disqualified_flagged_request_takes_its_own_launch_in_the_same_call(p, flags):
    """a flagged request of 12-element samples (no whole 8-element groups per sample; n = 24 IS whole groups, so without the
    flag it would be a pair row) among rows of the same n: no row -- its own stage_perp_kernel launch in the same call, which
    still projects, beside the others' one table launch; never a two-condition row, whose blend is linear"""
    from test_gpu_table_zstar import names_of
    sd, ed = PAIRS[p]
    t, _ = check_call(disqualified_cases(sd, ed), "a sample of 12 elements", flags=flags)
    assert t.host[:16].view(torch.int32).tolist()[2:] == [5, 1]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_perp_kernel_table" in n for n in names) == 1 and \
        sum("stage_perp_kernel<" in n for n in names) == 1, names


@gpu
@pytest.mark.parametrize("p", [0, 2, 4], ids=[PAIR_IDS[i] for i in (0, 2, 4)])
def test_the_anchors_beside_ordinary_rows(p):
    """a negative equal to the positive gives plain guidance, a sample with o_c == o_u gives a = 0: both in ONE launch beside an
    ordinary row, all with the bits of the double and of the request's own launch"""
    sd, ed = PAIRS[p]
    t, devs = check_call(anchor_cases(sd, ed), "the anchors")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [3, 1]
    F = torch.float32
    if sd is F and ed is F:                                        # the anchors that need no double: a DENOISE stage stores gd
        P = 4104
        _, same, zero = devs
        e0, e1 = (PG.values(same.pristine[k], F) for k in ("e0", "e1"))
        want = PG.bits(e1 + torch.tensor(7.5, dtype=F) * (e0 - e1), F)
        for name in ("x_out", "m_out", "x_out2"):
            assert torch.equal(same.arenas[name].payload_bits().cpu(), want), name
        assert torch.equal(same.xo3.payload_bits().cpu(), want)
        e1, g = (PG.values(zero.pristine[k], F)[P:2 * P] for k in ("e1", "g"))
        want = PG.bits(e1 + torch.tensor(3.0, dtype=F) * (torch.zeros_like(e1) - torch.tensor(2.5, dtype=F) * (g - e1)), F)
        for name in ("x_out", "m_out", "x_out2"):
            assert torch.equal(zero.arenas[name].payload_bits().cpu()[P:2 * P], want), name
        assert torch.equal(zero.xo3.payload_bits().cpu()[P:2 * P], want)


@gpu
def test_all_eight_flags_every_other_row_kind_beside_perp_rows():
    """one call that carries all eight table flags: the 29 requests of tests/test_gpu_table_kinds.py (plain / UniPC, MS3, SDE of
    two model types, thresholded of two ratios, mask-blend, ragged), two guidance-rescale rows, two APG rows (one with a
    momentum), CFG-Zero* rows, two-condition rows and Perp-Neg rows of two groups among them.  Every request the bits of its
    double; ONE table kernel per run, by name; the header counts the runs"""
    import apg_guarded as AG
    import test_gpu_table_apg as TA
    import test_gpu_table_kinds as TK
    import test_gpu_table_pair as TP
    import test_gpu_table_rescale as TR
    import test_gpu_table_zstar as TZ
    from test_gpu_edges import PAIRS as EPAIRS
    from test_gpu_table import TableCall
    p, ci = 4, 0
    sd, ed = EPAIRS[p]
    kcases, kwants = TK.build(TK.KINDS, p, ci)
    rsc = TR.requests(2, 4104, 2, sd, ed, "noise", True, seed=2)
    apg = TA.requests(2, 4104, 1, sd, ed, "noise", seed=1)
    zs = TZ.requests(2, 4104, 2, sd, ed, "v", True, seed=4)
    pr = TP.requests(2, 4104, sd, ed, seed=4, only=("v", True))
    na = requests(3, 4104, 2, sd, ed, "v", True, seed=4)
    nb = requests(2, 8, 3, sd, ed, "noise", False, seed=6)
    ks = [("k", c, w) for c, w in zip(kcases, kwants)]
    order = (ks[:5] + [("n", na[0], None), ("r", rsc[0], None), ("a", apg[0], None), ("p", pr[0], None)] + ks[5:20]
             + [("n", nb[0], None), ("z", zs[0], None), ("n", na[1], None), ("a", apg[1], None)] + ks[20:]
             + [("r", rsc[1], None), ("n", nb[1], None), ("z", zs[1], None), ("p", pr[1], None), ("n", na[2], None)])
    wants, devs = [], []
    for kind, c, w in order:
        wants.append(w if kind == "k" else run_double(c) if kind == "n" else TP.run_double(c) if kind == "p"
                     else TZ.run_double(c) if kind == "z" else TR.run_double(c) if kind == "r" else TA.run_double(c))
        if kind == "a":
            d = AG.on(c, DEV)
            d.b.thr_hint = d.avg.ptr
            devs.append(d)
        else:
            devs.append(c.on(DEV))
    t = TableCall(devs, flags=ALL8)
    assert t.host.numel() == L.table_bytes(len(devs), ALL8) == L.table_bytes(len(devs), ALL8 & ~PP)
    t.tick()
    for (kind, _, _), d, w in zip(order, devs, wants):
        if kind == "a":
            AG.verify(d, w)
        else:
            d.verify(w)
    assert t.table_intact(), "the kernels may only read their table"
    kruns = TK.runs_of(TK.KINDS, TK.ALL)
    n_runs = len(kruns) + 1 + 1 + 1 + 1 + 2                        # + rescale, APG, CFG-Zero*, two-condition, two Perp-Neg groups
    assert t.host[:16].view(torch.int32).tolist() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(devs), n_runs]
    names = TZ.names_of(t.tick)
    fam = lambda s: sum(s in n for n in names)
    assert fam("stage_perp_kernel_table") == 2 and fam("stage_perp_kernel<") == 0
    assert fam("stage_pair_kernel_table") == 1 and fam("stage_pair_kernel<") == 0
    assert fam("stage_zstar_kernel_table") == 1 and fam("stage_rescale_kernel_table") == 1 and fam("stage_apg_kernel_table") == 1
    for kind, family in TK.FAMILY.items():
        assert fam(family + "<") == sum(1 for k, _ in kruns if k == kind), (kind, names)
    n_fused, n_lone = TK.lone_launches(TK.KINDS, TK.ALL)
    assert len(names) == n_runs + n_fused + n_lone, names          # one kernel launch per run, the rest as mode 0 launches them
