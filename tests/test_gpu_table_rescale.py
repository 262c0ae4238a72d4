"""Guidance-rescale rows of the table-driven launch (DPM_TABLE_RESCALE, stage_rescale_kernel_table) on the MI355X.  Kernel
level, through the C ABI and between guards (tests/guarded.py), with the cases of tests/test_gpu_cfg_rescale.py: DPM_TABLE_FILL |
DPM_TABLE_RESCALE into a host tensor, `copy_` to the device, DPM_TABLE_LAUNCH | DPM_TABLE_RESCALE.  Every request must get the
bits of its own dpm_stage_launch AND of the numpy double (tests/rescale_double.py, whose inputs are checked decidable on the CPU
first: f does not depend on the summation order); the table and its guards must be intact; the launches are counted by name.
The shapes are the smallest at which this kernel can go wrong: samples of 8 elements (one group), 4096 (one full iteration of
512 threads x 8), 4104 (a ragged second one), 16384 (the largest the register path holds) and 16392 (the re-read path); groups
of 1, 2 and 17 rows; 1 and 3 samples per row; LIN1 / TWO / MS3 / DENOISE, STORE_M, the duplicate store, phi and the guidance
scale differ from row to row, model type and DPM_F_TO_X0 from group to group.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import guarded as G
from dpm_solver_amd import _lib as L
from test_gpu_cfg_rescale import MODELS, PAIRS, PAIR_IDS, _Pristine, make_case, run_double
from test_gpu_table import DEV, TableCall, _stream

gpu = pytest.mark.gpu
RSC = L.TABLE_RESCALE
FORMS = ("LIN1", "TWO", "MS3", "DENOISE")
PARAMS = [(0.7, 1.5), (1.0, 7.5), (0.7, 7.5), (1.0, 1.5)]       # (phi, guidance scale)
# (rows, elements per sample, samples per row): every size with every group size, both batches at every size and group size
CELLS = [(1, 8, 1), (2, 8, 3), (17, 8, 3), (17, 8, 1),
         (1, 4096, 3), (2, 4096, 1), (17, 4096, 1),
         (1, 4104, 1), (2, 4104, 3), (17, 4104, 3),
         (1, 16384, 3), (2, 16384, 1), (17, 16384, 1),
         (1, 16392, 1), (2, 16392, 3), (17, 16392, 1)]
CELL_IDS = ["%drow-per%d-b%d" % c for c in CELLS]


def group_of(p, ci):
    """(model type, DPM_F_TO_X0) of dtype pair p at CELLS[ci]: what a group shares"""
    q = 3 * p + ci
    return MODELS[q % 4], (q // 4) % 2 == 0


def test_cells_cover_sizes_groups_batches_and_network_kinds():
    assert {c[1] for c in CELLS} == {8, 4096, 4104, 16384, 16392} and len(PAIRS) == 5
    for P in {c[1] for c in CELLS}:
        assert {c[0] for c in CELLS if c[1] == P} == {1, 2, 17} and {c[2] for c in CELLS if c[1] == P} == {1, 3}
    for count in (1, 2, 17):
        assert {c[2] for c in CELLS if c[0] == count} == {1, 3}
    for p in range(5):
        assert {group_of(p, ci) for ci in range(len(CELLS))} == {(m, t) for m in MODELS for t in (True, False)}


def requests(count, P, batch, sd, ed, model, tox0, seed=0, forms=FORMS):
    """the CPU cases of one per-request-stage call: the forms in rotation, every row with a record of its own -- STORE_M, the
    duplicate store, phi and the guidance scale differ from row to row"""
    out = []
    for r in range(count):
        q = r + seed
        v = dict(form=forms[q % len(forms)], model=model, tox0=tox0, store_m=q % 3 != 0, dup=q % 4 != 3,
                 phi=PARAMS[q % 4][0], s=PARAMS[(q // 2) % 4][1])
        out.append(make_case(v, P, batch, sd, ed, seed=seed, req=r, per_request=True))
    return out


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_inputs_of_every_case_are_decidable(p):
    """the doubles of the whole sweep on the CPU: none of its samples has an f that depends on the summation order -- the
    precondition under which the GPU tests ask for equal bits (rescale_double.assert_inputs_decidable)"""
    sd, ed = PAIRS[p]
    for ci, (count, P, batch) in enumerate(CELLS):
        for c in requests(count, P, batch, sd, ed, *group_of(p, ci), seed=7 * p + ci):
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


def check_call(cases, what, check_own=True):
    """one FILL / copy / LAUNCH tick with the flag on guarded operands: guards, inputs and bits against the double (verify), the
    table and its guards as the host wrote them, then every request's own dpm_stage_launch into the same, refilled, output
    arenas: the same bits, guards included"""
    wants, devs = [run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = TableCall(devs, flags=RSC)
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
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=CELL_IDS)
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_rescale_table_calls_equal_the_single_launches_and_the_double(p, ci):
    sd, ed = PAIRS[p]
    count, P, batch = CELLS[ci]
    model, tox0 = group_of(p, ci)
    cases = requests(count, P, batch, sd, ed, model, tox0, seed=7 * p + ci)
    t, _, _ = check_call(cases, (model, tox0, count, P, batch))
    header = t.host[:16].view(torch.int32).tolist()
    assert header == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1], header


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_one_launch_per_group_counted_by_kernel_name(sdt):
    # a group of ONE, of 17 and of 40 rescale rows, every form, phi and scale among them: ONE stage_rescale_kernel_table launch
    for count in (1, 17, 40):
        t = TableCall([c.on(DEV) for c in requests(count, 4104, 1, sdt, sdt, "noise", True, seed=count)], flags=RSC)
        names = names_of(t.tick)
        assert len(names) == 1 and "stage_rescale_kernel_table" in names[0], (count, names)
    # 20 rescale + 20 plain requests: two runs, one launch of either table family
    cases = requests(40, 4104, 1, sdt, sdt, "noise", True, seed=3, forms=("LIN1", "TWO", "MS3"))
    for c in cases[::2]:
        c.st.flags &= ~L.F_CFG_RESCALE
        c.st.cg_scale = c.st.cfg_scale * c.st.sigma_e
    cases = [c.on("cpu") for c in cases]
    t, _, _ = check_call(cases, "rescale beside plain", check_own=False)
    assert t.host[:16].view(torch.int32).tolist()[2:] == [40, 2]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_rescale_kernel_table" in n for n in names) == 1 and \
        sum("stage_kernel_table<" in n for n in names) == 1, names
    # without the flag the same rescale requests are launched one by one, as in version 212
    t = TableCall([c.on(DEV) for c in requests(5, 4104, 1, sdt, sdt, "noise", True, seed=5)], flags=RSC)
    names = names_of(lambda: t.tick(flags=0))
    assert len(names) == 5 and all("stage_rescale_kernel<" in n for n in names), names


@gpu
@pytest.mark.parametrize("p", [0, 2, 4], ids=[PAIR_IDS[i] for i in (0, 2, 4)])
def test_a_disqualified_row_takes_its_own_launch_in_the_same_call(p):
    """a flagged request of 12-element samples (no whole 8-element groups) among rows of the same n: no row -- its own
    stage_rescale_kernel launch in the same call, which still rescales, beside the others' one table launch"""
    sd, ed = PAIRS[p]
    cases = requests(4, 8, 3, sd, ed, "v", True, seed=11)
    cases.insert(2, requests(3, 12, 2, sd, ed, "v", True, seed=11)[2])
    t, _, _ = check_call(cases, "a sample of 12 elements")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [5, 1]
    names = names_of(t.tick)
    assert len(names) == 2 and sum("stage_rescale_kernel_table" in n for n in names) == 1 and \
        sum("stage_rescale_kernel<" in n for n in names) == 1, names


@gpu
@pytest.mark.parametrize("p", [0, 1, 3, 4], ids=[PAIR_IDS[i] for i in (0, 1, 3, 4)])
def test_a_constant_sample_is_non_finite_and_its_neighbours_are_exact(p):
    """std_g == 0 gives what IEEE gives in every element of THAT sample; the other samples of its row and the other rows of the
    same launch keep the bits of the double"""
    import kernel_double as KD
    import rescale_double as RD
    sd, ed = PAIRS[p]
    P = 4104
    cases = requests(3, P, 3, sd, ed, "noise", p % 2 == 0, seed=9)
    pr = dict(cases[1].pristine)
    const = torch.full((P,), 0.25).to(ed).view(G._INT[2 if ed is not torch.float32 else 4])
    for name in ("e0", "e1"):
        bits = pr[name].clone()
        bits[P:2 * P] = const                                                 # sample 1 of row 1: e0 == e1 == constant
        pr[name] = bits
    cases[1] = make_case(dict(form="TWO", model="noise", tox0=p % 2 == 0, store_m=True, dup=True, phi=0.7, s=7.5), P, 3, sd, ed,
                         seed=9, req=1, per_request=True, like=_Pristine(pr))
    wants = [run_double(cases[0]), cases[1], run_double(cases[2])]
    assert RD.launch_raw_double(KD._Ref(cases[1].st), KD._Ref(cases[1].b)) == 0
    devs = [c.on(DEV) for c in cases]
    t = TableCall(devs, flags=RSC)
    t.tick()
    assert t.table_intact() and t.host[:16].view(torch.int32).tolist()[2:] == [3, 1]
    devs[0].verify(wants[0])
    devs[2].verify(wants[2])
    devs[1].verify()                                                          # guards, inputs, every payload element stored
    for name in ("x_out", "m_out", "x_out2"):
        got, want = devs[1].arenas[name].payload_bits().cpu(), cases[1].arenas[name].payload_bits()
        assert not torch.isfinite(devs[1].arenas[name].payload()[P:2 * P].float()).any(), name
        assert not torch.isfinite(cases[1].arenas[name].payload()[P:2 * P].float()).any(), name
        assert torch.equal(got[:P], want[:P]) and torch.equal(got[2 * P:], want[2 * P:]), name
