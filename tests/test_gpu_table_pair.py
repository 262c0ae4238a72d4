"""Two-condition rows of the table-driven launch (DPM_TABLE_PAIR, stage_pair_kernel_table) on the MI355X.  Kernel level, through
the C ABI and between guards (tests/pair_guarded.py): DPM_TABLE_FILL | DPM_TABLE_PAIR into a host tensor, `copy_` to the device,
DPM_TABLE_LAUNCH | DPM_TABLE_PAIR.  Every request must get the bits of its own dpm_stage_launch (mode 0, no copies) AND of the
numpy double (tests/table_pair_double.py) -- the arithmetic is elementwise, so there is no tolerance and no precondition --, both
copies must equal x_out, and every guard band, the third copy's and the table's included, must be intact.
The shapes are the plain table family's (tests/test_gpu_table.py): groups of 1, 2, 17 and 33 rows; n = 8 (one group), 2040 (a
short tile with clamped lanes), 2048 (exactly one tile), 2056 (one tile plus one group), 4104 and 16384; and 200 rows of 8 and of
2056 elements.  LIN1 / TWO / MS3 / DENOISE share a group; the four model types, both DPM_F_TO_X0 settings, DPM_F_STORE_M, both
scales and rows with and without the copies differ from row to row.  fp16/fp16 and fp32/fp32 run every cell, the other three
dtype pairs (17, 2056) and (33, 8).
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import guarded as G
import kernel_double as KD
import pair_guarded as PG
import table_pair_double as TPD
from dpm_solver_amd import _lib as L
from test_gpu_cfg_pair import MODELS, PAIR_IDS, PAIRS, make_stage

gpu = pytest.mark.gpu
DEV = "cuda:0"
PR = L.TABLE_PAIR
ALL7 = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND | L.TABLE_RESCALE | L.TABLE_APG | L.TABLE_ZSTAR | PR
FORMS = ("LIN1", "TWO", "MS3", "DENOISE")
CELLS = [(c, n) for c in (1, 2, 17, 33) for n in (8, 2040, 2048, 2056, 4104, 16384)] + [(200, 8), (200, 2056)]
FULL, FEW = (0, 3), (1, 2, 4)                       # fp32/fp32 and fp16/fp16: every cell; the other pairs: two cells
SWEEP = [(p, c, n) for p in FULL for c, n in CELLS] + [(p, c, n) for p in FEW for c, n in ((17, 2056), (33, 8))]
SWEEP_IDS = ["%s-%drow-n%d" % (PAIR_IDS[p], c, n) for p, c, n in SWEEP]


def variant(q):
    """the record of row q of a call: everything differs from row to row"""
    return dict(form=FORMS[q % 4], model=MODELS[(q // 4) % 4], tox0=q % 3 != 0, store_m=q % 5 < 3, copies=q % 7 not in (2, 5),
                s=(1.0 + 0.037 * q, -2.0 + 0.029 * q))


class PairRow(PG.PairLaunch):
    """a PairLaunch that may name the two copies: x_out2 (GuardedLaunch's `dup`) and a THIRD copy in an arena of its own, which
    the record carries in thr_hint as a DPM_TABLE_PAIR call reads it"""

    def __init__(self, st, n, sd, ed, copies=False, device="cpu", like=None, **kw):
        kw["dup"] = copies
        super().__init__("pair-table", st, n, sd, ed, device=device, like=like, **kw)
        self.copies = copies
        self.xo3 = G.Arena(sd, self.n, device, self.offset)
        if copies:
            self.b.thr_hint = self.xo3.ptr

    def on(self, device, copies=None):
        kw = dict(self.kw)
        kw.pop("dup")
        return PairRow(self.st, self.n, self.sd, self.ed, copies=self.copies if copies is None else copies, device=device,
                       like=self, **kw)

    def verify(self, want=None, rc=0, noop=False):
        super().verify(want, rc, noop)
        what = "third copy of request %d (n=%d)" % (self.req, self.n)
        if self.copies and rc == 0 and not noop:
            self.xo3.verify(what, self.arenas["x_out"].payload_bits())         # equal to x_out, guards intact
            assert torch.equal(self.arenas["x_out2"].payload_bits(), self.arenas["x_out"].payload_bits()), what
        else:
            self.xo3.verify(what)                                               # nothing may write it


def requests(count, n, sd, ed, seed=0, only=None):
    """the CPU cases of one per-request-stage call; only=(model, tox0): one group"""
    out = []
    for r in range(count):
        v = variant(r + seed)
        if only is not None:
            v = dict(v, model=only[0], tox0=only[1])
        out.append(PairRow(make_stage(v, seed * 131 + r), n, sd, ed, copies=v["copies"], seed=seed, req=r, per_request_stages=True))
    return out


def run_double(case):
    """the table call's double on one CPU case: the stage, then the copies"""
    assert TPD.launch_raw(KD._Ref(case.st), KD._Ref(case.b), None, copies=True) == 0
    case.verify()
    return case


def runs_of(cases):
    return len({(c.st.model_type, c.st.flags & L.F_TO_X0) for c in cases})


def test_cells_cover_sizes_groups_forms_and_network_kinds():
    assert (PAIRS[0], PAIRS[3]) == ((torch.float32, torch.float32), (torch.float16, torch.float16)) and len(PAIRS) == 5
    assert {n for _, n in CELLS} == {8, 2040, 2048, 2056, 4104, 16384} and {c for c, _ in CELLS} == {1, 2, 17, 33, 200}
    assert len(SWEEP) == 2 * 26 + 3 * 2
    rows = [variant(q) for q in range(17)]
    assert {v["form"] for v in rows} == set(FORMS) and {v["model"] for v in rows} == set(MODELS)
    assert {v["tox0"] for v in rows} == {True, False} and {v["store_m"] for v in rows} == {True, False}
    assert {v["copies"] for v in rows} == {True, False} and len({v["s"] for v in rows}) == 17
    for m in MODELS:                                               # one group holds several forms
        assert len({v["form"] for v in [variant(q) for q in range(33)] if v["model"] == m and v["tox0"]}) >= 3


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_the_double_stays_inside_its_payloads(p):
    """the doubles of the sweep's smaller cells on the CPU: every named output written, copies equal, no guard touched"""
    sd, ed = PAIRS[p]
    for pp, count, n in SWEEP:
        if pp == p and count <= 17 and n <= 2056:
            for c in requests(count, n, sd, ed, seed=count + n):
                run_double(c)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_call(cases, what, flags=PR):
    """one FILL / copy / LAUNCH tick with the flag on guarded operands: guards, inputs, bits against the double and the copies
    (verify), the table and its guards as the host wrote them, then every request's own dpm_stage_launch -- mode 0, no copies --
    on the same inputs: the same bits in x_out and m_out"""
    from test_gpu_table import TableCall
    wants, devs = [run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = TableCall(devs, flags=flags)
    assert t.host.numel() == L.table_bytes(len(cases), flags)
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
@pytest.mark.parametrize("p,count,n", SWEEP, ids=SWEEP_IDS)
def test_pair_table_calls_equal_the_single_launches_and_the_double(p, count, n):
    sd, ed = PAIRS[p]
    cases = requests(count, n, sd, ed, seed=7 * p + count + n)
    t, _ = check_call(cases, (count, n))
    header = t.host[:16].view(torch.int32).tolist()
    assert header == [L.TABLE_MAGIC, L.lib.dpm_version(), count, runs_of(cases)], header


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_one_launch_per_group_counted_by_kernel_name(sdt):
    from test_gpu_table import TableCall
    from test_gpu_table_zstar import names_of
    for count in (1, 17, 40):                                      # ONE group, every form and both kinds of row in it: ONE launch
        t = TableCall([c.on(DEV) for c in requests(count, 4104, sdt, sdt, seed=count, only=("noise", True))], flags=PR)
        names = names_of(t.tick)
        assert len(names) == 1 and "stage_pair_kernel_table" in names[0], (count, names)
    # without bit 16384 the same requests -- without copies: the lone kernel has no second store -- are launched one by one
    cases = [c.on(DEV, copies=False) for c in requests(5, 4104, sdt, sdt, seed=5, only=("v", True))]
    t = TableCall(cases, flags=PR)
    names = names_of(lambda: t.tick(flags=0))
    assert len(names) == 5 and all("stage_pair_kernel<" in n for n in names), names


@gpu
def test_a_request_without_a_row_takes_its_own_launch_in_the_same_call():
    """a request of 2052 elements (n % 8 != 0: no whole 8-element groups) without copies among rows: its own
    stage_pair_kernel launch beside the others' one table launch"""
    from test_gpu_table_zstar import names_of
    sd = ed = torch.float16
    cases = requests(4, 2056, sd, ed, seed=11, only=("noise", True))
    odd = PairRow(make_stage(dict(variant(2), model="noise", tox0=True), 99), 2052, sd, ed, copies=False, seed=11, req=9,
                  per_request_stages=True)
    cases.insert(2, odd)
    t, _ = check_call(cases, "n % 8 != 0")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [5, 1]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_pair_kernel_table" in n for n in names) == 1 and \
        sum("stage_pair_kernel<" in n for n in names) == 1, names


@gpu
def test_all_seven_flags_every_other_row_kind_beside_pair_rows():
    """one call that carries all seven table flags: the 29 requests of tests/test_gpu_table_kinds.py (plain / UniPC, MS3, SDE of
    two model types, thresholded of two ratios, mask-blend, ragged), two guidance-rescale rows, two APG rows (one with a
    momentum), CFG-Zero* rows and two-condition rows of two groups among them.  Every request the bits of its double; ONE table
    kernel per run, by name; the header counts the runs"""
    import apg_guarded as AG
    import test_gpu_table_apg as TA
    import test_gpu_table_kinds as TK
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
    pa = requests(3, 4104, sd, ed, seed=4, only=("v", True))
    pb = requests(2, 8, sd, ed, seed=6, only=("noise", False))
    ks = [("k", c, w) for c, w in zip(kcases, kwants)]
    order = (ks[:5] + [("p", pa[0], None), ("r", rsc[0], None), ("a", apg[0], None)] + ks[5:20]
             + [("p", pb[0], None), ("z", zs[0], None), ("p", pa[1], None), ("a", apg[1], None)] + ks[20:]
             + [("r", rsc[1], None), ("p", pb[1], None), ("z", zs[1], None), ("p", pa[2], None)])
    wants, devs = [], []
    for kind, c, w in order:
        wants.append(w if kind == "k" else run_double(c) if kind == "p" else TZ.run_double(c) if kind == "z"
                     else TR.run_double(c) if kind == "r" else TA.run_double(c))
        if kind == "a":
            d = AG.on(c, DEV)
            d.b.thr_hint = d.avg.ptr
            devs.append(d)
        else:
            devs.append(c.on(DEV))
    t = TableCall(devs, flags=ALL7)
    assert t.host.numel() == L.table_bytes(len(devs), ALL7) == L.table_bytes(len(devs), ALL7 & ~PR) + len(devs) * L.TABLE_PAIR_BYTES
    t.tick()
    for (kind, _, _), d, w in zip(order, devs, wants):
        if kind == "a":
            AG.verify(d, w)
        else:
            d.verify(w)
    assert t.table_intact(), "the kernels may only read their table"
    kruns = TK.runs_of(TK.KINDS, TK.ALL)
    n_runs = len(kruns) + 1 + 1 + 1 + 2                            # + rescale, APG, CFG-Zero*, two two-condition groups
    assert t.host[:16].view(torch.int32).tolist() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(devs), n_runs]
    names = TZ.names_of(t.tick)
    fam = lambda s: sum(s in n for n in names)
    assert fam("stage_pair_kernel_table") == 2 and fam("stage_pair_kernel<") == 0
    assert fam("stage_zstar_kernel_table") == 1 and fam("stage_rescale_kernel_table") == 1 and fam("stage_apg_kernel_table") == 1
    for kind, family in TK.FAMILY.items():
        assert fam(family + "<") == sum(1 for k, _ in kruns if k == kind), (kind, names)
    n_fused, n_lone = TK.lone_launches(TK.KINDS, TK.ALL)
    assert len(names) == n_runs + n_fused + n_lone, names          # one kernel launch per run, the rest as mode 0 launches them
