"""Adaptive-projected-guidance rows of the table-driven launch (DPM_TABLE_APG, stage_apg_kernel_table) on the MI355X.  Kernel
level, through the C ABI and between guards (tests/guarded.py, the fp32 running average in an arena of its own:
tests/apg_guarded.py), with the cases of tests/test_gpu_cfg_apg.py: DPM_TABLE_FILL | DPM_TABLE_APG into a host tensor, `copy_` to
the device, DPM_TABLE_LAUNCH | DPM_TABLE_APG, the running average of every request in dpm_buffers.thr_hint.  Every request must
get the bits of its own dpm_stage_launch (the average in workspace) AND of the numpy double (tests/apg_double.py, whose inputs
are checked decidable on the CPU first: sc and q do not depend on the summation order) -- the outputs and, with a momentum, the
stored average; without a momentum the poisoned average arena is untouched; the table and its guards must be intact; the
launches are counted by name.
The shapes are the smallest at which this kernel can go wrong: samples of 8 elements (one group), 4096 (one full iteration of
512 threads x 8), 4104 (a ragged second one), 16384 (the largest the register path holds) and 16392 (the re-read path); groups
of 1, 2 and 17 rows; 1 and 3 samples per row; LIN1 / TWO / MS3 / DENOISE, STORE_M, the duplicate store, eta, r, beta and the
guidance scale differ from row to row, the model type from group to group.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import apg_guarded as AG
import guarded as G
from dpm_solver_amd import _lib as L
from test_gpu_cfg_apg import BETAS, ETAS, MODELS, PAIRS, PAIR_IDS, RS, make_case, run_double
from test_gpu_table import DEV, TableCall, _stream

gpu = pytest.mark.gpu
APG = L.TABLE_APG
FORMS = ("LIN1", "TWO", "MS3", "DENOISE")
SCALES = (7.5, 1.5, 3.0)
# (rows, elements per sample, samples per row): every size with every group size, both batches at every size and group size
CELLS = [(1, 8, 1), (2, 8, 3), (17, 8, 3), (17, 8, 1),
         (1, 4096, 3), (2, 4096, 1), (17, 4096, 1),
         (1, 4104, 1), (2, 4104, 3), (17, 4104, 3),
         (1, 16384, 3), (2, 16384, 1), (17, 16384, 1),
         (1, 16392, 1), (2, 16392, 3), (17, 16392, 1)]
CELL_IDS = ["%drow-per%d-b%d" % c for c in CELLS]


def seed_of(p, ci):
    return 7 * p + ci


def group_of(p, ci):
    """the model type of dtype pair p at CELLS[ci]: what a group shares"""
    return MODELS[(3 * p + ci) % 4]


def variant(q, model, forms=FORMS):
    """the record of row q of a call: form, STORE_M, the duplicate store, eta, r, beta and the scale all differ from row to row"""
    return dict(form=forms[q % len(forms)], model=model, store_m=q % 3 != 0, dup=q % 4 != 3, eta=ETAS[q % 3], r=RS[(q // 3) % 3],
                beta=BETAS[(q // 2) % 2], s=SCALES[(q // 2) % 3])


def requests(count, P, batch, sd, ed, model, seed=0, forms=FORMS):
    """the CPU cases of one per-request-stage call, every row with a record of its own"""
    return [make_case(variant(r + seed, model, forms), P, batch, sd, ed, seed=seed, req=r, per_request=True) for r in range(count)]


def test_cells_cover_sizes_groups_batches_network_kinds_and_a_momentum_in_request_0():
    assert {c[1] for c in CELLS} == {8, 4096, 4104, 16384, 16392} and len(PAIRS) == 5
    for P in {c[1] for c in CELLS}:
        assert {c[0] for c in CELLS if c[1] == P} == {1, 2, 17} and {c[2] for c in CELLS if c[1] == P} == {1, 3}
        # request 0 carries a momentum in at least one cell of this size, and none in another
        first = {variant(seed_of(p, ci), "noise")["beta"] != 0 for p in range(5) for ci, c in enumerate(CELLS) if c[1] == P}
        assert first == {True, False}, P
    for count in (1, 2, 17):
        assert {c[2] for c in CELLS if c[0] == count} == {1, 3}
    for p in range(5):
        assert {group_of(p, ci) for ci in range(len(CELLS))} == set(MODELS)
    rows = [variant(q, "noise") for q in range(36)]
    assert {(v["eta"], v["r"], v["beta"]) for v in rows} == {(e, r, b) for e in ETAS for r in RS for b in BETAS}
    assert {v["form"] for v in rows[:17]} == set(FORMS) and {v["store_m"] for v in rows[:17]} == {True, False}
    assert {v["dup"] for v in rows[:17]} == {True, False} and {v["s"] for v in rows[:17]} == set(SCALES)


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_inputs_of_every_case_are_decidable(p):
    """the doubles of the whole sweep on the CPU: none of its samples has an sc or a q that depends on the summation order --
    the precondition under which the GPU tests ask for equal bits (apg_double.assert_inputs_decidable).  No case is dropped."""
    sd, ed = PAIRS[p]
    for ci, (count, P, batch) in enumerate(CELLS):
        for c in requests(count, P, batch, sd, ed, group_of(p, ci), seed=seed_of(p, ci)):
            run_double(c)


def mixed_cases(sdt):
    """20 APG + 20 plain requests of one call (the plain ones: the flag cleared, the planner's fields)"""
    cases = requests(40, 4104, 1, sdt, sdt, "noise", seed=3, forms=("LIN1", "TWO", "MS3"))
    for c in cases[::2]:
        c.st.flags &= ~L.F_CFG_APG
        c.st.cg_scale, c.st.thr_ratio, c.st.thr_max = c.st.cfg_scale * c.st.sigma_e, 0.0, 0.0
    return cases


def disqualified_cases(sd, ed):
    """four rows of 8-element samples and, in the middle, a flagged request of 12-element samples with a momentum"""
    cases = requests(4, 8, 3, sd, ed, "v", seed=10)
    cases.insert(2, make_case(dict(variant(2, "v"), beta=-0.5), 12, 2, sd, ed, seed=10, req=7, per_request=True))
    return cases


def test_inputs_of_the_other_calls_are_decidable():
    """... and those of the calls outside the sweep that are compared with the double on the GPU"""
    for sdt in (torch.float16, torch.float32):
        for c in mixed_cases(sdt):
            run_double(c)
    for p in (0, 2, 4):
        for c in disqualified_cases(*PAIRS[p]):
            run_double(c)


def names_of(fn):
    """names of the stage kernels fn() launches, one entry per launch (torch's profiler)"""
    from torch.profiler import ProfilerActivity, profile
    fn()                                                          # (first-launch costs outside the profile)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if "stage_" in e.key and "kernel" in e.key for _ in range(e.count)]


def on_device(cases):
    """the cases on the GPU, the running average of each named by thr_hint too: what a DPM_TABLE_APG call reads (workspace,
    which the request's own dpm_stage_launch reads, stays; request 0's becomes the table inside the call)"""
    devs = [AG.on(c, DEV) for c in cases]
    for d in devs:
        d.b.thr_hint = d.avg.ptr
    return devs


def check_call(cases, what, check_own=True):
    """one FILL / copy / LAUNCH tick with the flag on guarded operands: guards, inputs and bits against the double -- outputs
    and the average (AG.verify) --, the table and its guards as the host wrote them, then every request's own dpm_stage_launch
    on the pristine average into the same, refilled, output arenas: the same bits, guards included, the average's too"""
    wants, devs = [run_double(c) for c in cases], on_device(cases)
    t = TableCall(devs, flags=APG)
    t.tick()
    for d, w in zip(devs, wants):
        AG.verify(d, w)
    assert t.table_intact(), (what, "the kernel may only read its table")
    for r, d in enumerate(devs if check_own else ()):
        fused = {k: d.arenas[k].raw.clone() for k in G.OUTPUTS}
        fused_avg = d.avg.raw.clone()
        for k in G.OUTPUTS:
            d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])
        d.avg.raw.copy_(d.avg.before)                             # the average the request started from
        assert d.b.workspace == d.avg.ptr
        rc = L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
        for k in G.OUTPUTS:
            assert torch.equal(fused[k], d.arenas[k].raw), (what, r, d.n, k, "differs from the request's own dpm_stage_launch")
        assert torch.equal(fused_avg, d.avg.raw), (what, r, d.n, "the average differs from the request's own dpm_stage_launch")
    return t, devs, wants


@gpu
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=CELL_IDS)
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_apg_table_calls_equal_the_single_launches_and_the_double(p, ci):
    sd, ed = PAIRS[p]
    count, P, batch = CELLS[ci]
    model = group_of(p, ci)
    cases = requests(count, P, batch, sd, ed, model, seed=seed_of(p, ci))
    t, _, _ = check_call(cases, (model, count, P, batch))
    header = t.host[:16].view(torch.int32).tolist()
    assert header == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1], header


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_one_launch_per_group_counted_by_kernel_name(sdt):
    # a group of ONE, of 17 and of 40 APG rows, every form, eta, r, beta and scale among them: ONE stage_apg_kernel_table launch
    for count in (1, 17, 40):
        t = TableCall(on_device(requests(count, 4104, 1, sdt, sdt, "noise", seed=count)), flags=APG)
        names = names_of(t.tick)
        assert len(names) == 1 and "stage_apg_kernel_table" in names[0], (count, names)
    # 20 APG + 20 plain requests: two runs, one launch of either table family
    t, _, _ = check_call(mixed_cases(sdt), "APG beside plain", check_own=False)
    assert t.host[:16].view(torch.int32).tolist()[2:] == [40, 2]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_apg_kernel_table" in n for n in names) == 1 and \
        sum("stage_kernel_table<" in n for n in names) == 1, names
    # without bit 512 the same APG requests are launched one by one, as in version 214 (request 0 without a momentum: its
    # workspace is the table)
    cases = requests(5, 4104, 1, sdt, sdt, "noise", seed=4)
    assert cases[0].st.thr_max == 0.0 and any(c.st.thr_max != 0.0 for c in cases)
    t = TableCall(on_device(cases), flags=APG)
    names = names_of(lambda: t.tick(flags=0))
    assert len(names) == 5 and all("stage_apg_kernel<" in n for n in names), names


@gpu
@pytest.mark.parametrize("p", [0, 2, 4], ids=[PAIR_IDS[i] for i in (0, 2, 4)])
def test_a_disqualified_row_takes_its_own_launch_in_the_same_call(p):
    """a flagged request of 12-element samples (no whole 8-element groups), with a momentum, among rows of the same n: no row --
    its own stage_apg_kernel launch in the same call, on a copy of its buffers whose workspace is its thr_hint, which still
    projects and still advances its average, beside the others' one table launch"""
    sd, ed = PAIRS[p]
    t, devs, _ = check_call(disqualified_cases(sd, ed), "a sample of 12 elements")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [5, 1]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_apg_kernel_table" in n for n in names) == 1 and \
        sum("stage_apg_kernel<" in n for n in names) == 1, names
