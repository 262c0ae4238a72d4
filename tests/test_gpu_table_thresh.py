"""Thresholded rows of the table-driven launch (DPM_TABLE_THRESH, stage_thresh_kernel_table) on the MI355X.  Kernel level,
through the C ABI and between guards (tests/guarded.py), as tests/test_gpu_table.py: DPM_TABLE_FILL | DPM_TABLE_THRESH into a
host tensor, `copy_` to the device, DPM_TABLE_LAUNCH | DPM_TABLE_THRESH.  Every request must get the bits of the numpy double
AND of its own dpm_stage_launch (a cluster with a workspace at these batch sizes); the table and its guards must be intact;
the launches are counted by kernel name.
The shapes are the smallest at which this kernel can go wrong: samples of 8, 2040, 2048, 2056 elements (around 512 threads x 4),
12280 and 12288 (the largest a row holds); 1, 2, 17 and 200 requests; batch 1 and 3; rows rotating over LIN1 / TWO / MS3 with
coefficients of their own (and, in a test of its own, the thresholded DENOISE stage among them), STORE_M on and off, x_out2 named or null under classifier-free guidance, and -- in a noise group --
an alpha the division-by-invariant guard rejects beside alphas it accepts, so one launch runs both prologues.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C
import struct

import pytest
import torch

import guarded as G
import test_gpu_edges as E
from dpm_solver_amd import _lib as L
from test_gpu_edges import PAIRS, PAIR_IDS
from test_gpu_table import DEV, TableCall, _stream

gpu = pytest.mark.gpu
THR = L.TABLE_THRESH
PERS = (8, 2040, 2048, 2056, 12280, 12288)
# (requests, elements per sample, samples per request)
CELLS = [(c, per, 1) for c in (1, 2, 17) for per in PERS] + [(200, 8, 1), (200, 2056, 1), (5, 2056, 3)]
# guidance x model x ratio (0.995: the top-K front end; 0.5: the general route; 1.0: lo == hi, the maximum), ratio innermost
COMBOS = [(g, m, q) for g in ("uncond", "classifier-free") for m in ("noise", "v") for q in (0.995, 0.5, 1.0)]
ALPHA_ALL_ONES = struct.unpack("f", struct.pack("I", 0x3F7FFFFF))[0]      # div_invariant_ok says no: the general prologue


def combo_of(p, ci):
    """the combo of dtype pair p at CELLS[ci]; the step per block of sample sizes moves every size through the three ratios"""
    return COMBOS[(5 * p + ci + ci // len(PERS)) % len(COMBOS)]


def test_rotation_covers_every_guidance_prologue_and_ratio_per_dtype_pair():
    assert len(COMBOS) == 12 and len(PAIRS) == 5 and len(CELLS) == 21
    for p in range(len(PAIRS)):
        assert {combo_of(p, ci) for ci in range(len(CELLS))} == set(COMBOS)
    for per in PERS:                                             # every sample size meets every ratio
        assert {combo_of(p, ci)[2] for p in range(len(PAIRS)) for ci, c in enumerate(CELLS) if c[1] == per} == {0.995, 0.5, 1.0}


def thr_requests(count, per, batch, sd, ed, guidance, model, ratio, max_val, seed=0, thresh=lambda r: True,
                 forms=("LIN1", "TWO", "MS3")):
    """the CPU cases of one per-request-stage call: forms in rotation, a record of its own per request, STORE_M and x_out2
    mixed, every fourth request of a noise group with an alpha the invariant-division guard rejects; each request carries the
    workspace its OWN launch needs (the table call reads none)"""
    out = []
    for r in range(count):
        form = forms[(r + seed) % len(forms)]
        st = E.make_stage(form, guidance, model, store_m=(r + seed) % 3 != 0, thresh=thresh(r), seed=seed * 131 + r)
        st.thr_ratio, st.thr_max = ratio, max_val
        if r % 4 == 1:
            st.alpha_e, st.sigma_e = ALPHA_ALL_ONES, 0.000345
        nb = int(L.lib.dpm_threshold_workspace_bytes(batch, per)) if thresh(r) else None
        out.append(G.GuardedLaunch("thrtab", st, per * batch, sd, ed, batch=batch, ws_bytes=nb, seed=seed, req=r,
                                   dup=(guidance == "classifier-free" and r % 4 != 3), per_request_stages=True))
    return out


class ThreshTableCall(TableCall):
    def tick(self, flag=THR):
        self.call(L.TABLE_FILL | flag, self.host)
        self.dev.copy_(self.host, non_blocking=True)
        self.call(L.TABLE_LAUNCH | flag, self.dev)
        torch.cuda.synchronize()


def check_thresh_table_call(cases, what, same_as_own=True):
    """check_table_call of tests/test_gpu_table.py with the flag on both calls"""
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = ThreshTableCall(devs)
    t.tick()
    G.verify_all(devs, wants)
    assert t.table_intact(), (what, "the kernel may only read its table")
    for r, d in enumerate(devs):
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
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=["%dreq-per%d-b%d" % c for c in CELLS])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_thresholded_table_calls_equal_the_single_launches_and_the_double(p, ci):
    sd, ed = PAIRS[p]
    count, per, batch = CELLS[ci]
    guidance, model, ratio = combo_of(p, ci)
    max_val = (0.25, 100.0)[(p + ci) % 2]                        # below and above the quantile of |x0| ~ |N(0, 1)| / alpha
    cases = thr_requests(count, per, batch, sd, ed, guidance, model, ratio, max_val, seed=7 * p + ci)
    t, _, _ = check_thresh_table_call(cases, (guidance, model, ratio, max_val, count, per, batch))
    header = t.host[:16].view(torch.int32).tolist()
    assert header == [L.TABLE_MAGIC, L.lib.dpm_version(), count, 1], header


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_small_samples_of_a_batch_stay_inside_their_sample(p):
    """batch > 1 with samples of 4, 8 and 12 elements: a workgroup's 4-element accesses end with its sample -- the guards
    behind the last sample, and the neighbouring samples' bits, say so -- and a request of ragged samples (4 x 10 elements:
    n is a multiple of 8, the sample is not one of 4) owns no row: its own launch in the same call, the right bits"""
    sd, ed = PAIRS[p]
    for ci, (per, batch, count) in enumerate(((8, 3, 5), (4, 2, 3), (12, 2, 17), (8, 3, 1))):
        guidance, model, ratio = combo_of(p, ci)
        cases = thr_requests(count, per, batch, sd, ed, guidance, model, ratio, (0.25, 100.0)[ci % 2], seed=40 + ci)
        t, _, _ = check_thresh_table_call(cases, ("small samples", per, batch, count))
        assert t.host[:16].view(torch.int32).tolist()[2:] == [count, 1]
    cases = thr_requests(3, 8, 5, sd, ed, "uncond", "noise", 0.995, 1.0, seed=50)
    cases.insert(1, thr_requests(2, 10, 4, sd, ed, "uncond", "noise", 0.995, 1.0, seed=50)[1])
    t, _, _ = check_thresh_table_call(cases, "ragged samples")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [4, 1]
    names = _names(t.tick)
    assert len(names) == 2 and sum("stage_thresh_kernel_table" in n for n in names) == 1, names


@gpu
@pytest.mark.parametrize("guidance", ["uncond", "classifier-free"])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_thresholded_denoise_rows_among_the_other_forms(p, guidance):
    """DPM_FORM_DENOISE + DPM_F_THRESH, the last stage of denoise_to_zero: rows of the same group as LIN1 / TWO / MS3, every one
    with the bits of the double and of its own launch (the catch-all stage_thresh_kernel)"""
    sd, ed = PAIRS[p]
    forms = ("LIN1", "DENOISE", "TWO", "DENOISE", "MS3")
    for ci, (per, batch, count, model) in enumerate(((2056, 1, 7, "noise"), (12288, 1, 5, "v"), (8, 3, 5, "noise"))):
        ratio = (0.995, 0.5, 1.0)[(p + ci) % 3]
        cases = thr_requests(count, per, batch, sd, ed, guidance, model, ratio, (0.25, 100.0)[(p + ci) % 2], seed=60 + ci, forms=forms)
        assert sum(c.st.form == L.FORM_DENOISE for c in cases) >= 2
        t, _, _ = check_thresh_table_call(cases, ("denoise", per, batch, count, model, ratio))
        assert t.host[:16].view(torch.int32).tolist()[2:] == [count, 1]
        names = _names(t.tick)
        assert len(names) == 1 and "stage_thresh_kernel_table" in names[0], names


def _with_inputs(case, edit):
    """the same case with its pristine input payloads edited (float tensors by operand name) before the arenas are built"""
    vals = {k: v.view(case.arenas[k].dtype).clone() for k, v in case.pristine.items()}
    edit(vals)
    for k, v in vals.items():
        case.pristine[k] = v.view(G._INT[v.element_size()])
    return case.on("cpu")


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("ratio", [0.995, 0.5, 1.0])
@pytest.mark.parametrize("data", ["all-equal", "ties"])
def test_plateaus_of_x0(data, ratio, sdt):
    """e0 = e1 = 0 makes x0 = x / alpha: with |x| one value, or one of four, the selected order statistic sits in a plateau of
    the whole sample, or a quarter of it (the candidate list overflows: the radix levels over the whole LDS)"""
    g = torch.Generator().manual_seed(11)

    def edit(v):
        sign = torch.randint(0, 2, v["x"].shape, generator=g) * 2 - 1
        mag = torch.tensor([0.25, 0.5, 1.5, 3.0])[torch.randint(0, 4, v["x"].shape, generator=g)] if data == "ties" else 1.5
        v["x"].copy_((sign * mag).to(v["x"].dtype))
        v["e0"].zero_()
        if "e1" in v:
            v["e1"].zero_()
    for per, guidance in ((12288, "uncond"), (2056, "classifier-free"), (8, "uncond")):
        cases = thr_requests(3, per, 1, sdt, sdt, guidance, "noise", ratio, 1.0, seed=per)
        check_thresh_table_call([_with_inputs(c, edit) for c in cases], (data, ratio, per))


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("ratio", [0.995, 0.5])
def test_a_single_nan_makes_its_sample_nan_and_leaves_the_neighbours(ratio, sdt):
    """torch.quantile of a sample that holds a NaN is NaN: every output element of THAT sample is NaN, as the double gives;
    the other samples of the request and the other requests keep their bits"""
    per, batch = 2056, 3
    cases = thr_requests(4, per, batch, sdt, sdt, "uncond", "noise", ratio, 1.0, seed=3)

    def edit(v):
        v["x"][per + 777] = float("nan")                          # sample 1 of request 2
    cases[2] = _with_inputs(cases[2], edit)
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    t = ThreshTableCall(devs)
    t.tick()
    assert t.table_intact()
    for r in (0, 1, 3):
        devs[r].verify(wants[r])
    devs[2].verify()                                              # guards, inputs, every payload element stored
    for k in ("x_out",) + (("m_out",) if devs[2].st.flags & L.F_STORE_M else ()):
        got, want = devs[2].arenas[k].payload().float(), wants[2].arenas[k].payload().float()
        assert bool(want[per:2 * per].isnan().all()) and bool(got[per:2 * per].isnan().all()), k
        for lo in (0, 2 * per):
            assert torch.equal(devs[2].arenas[k].payload_bits().cpu()[lo:lo + per], wants[2].arenas[k].payload_bits()[lo:lo + per]), (k, lo)


def _names(fn):
    """names of the stage kernels fn() launches, one entry per launch (torch's profiler, as test_gpu_unipc_pool._stage_kernels,
    which does not list the thresholding family)"""
    from torch.profiler import ProfilerActivity, profile
    fn()                                                          # (first-launch costs outside the profile)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if "stage_kernel" in e.key or "stage_thresh_kernel" in e.key for _ in range(e.count)]


@gpu
@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_one_launch_per_group_counted_by_kernel_name(sdt):
    # a group of ONE, of 17 and of 200 thresholded requests: one stage_thresh_kernel_table launch each
    for count in (1, 17, 200):
        t = ThreshTableCall([c.on(DEV) for c in thr_requests(count, 2056, 1, sdt, sdt, "uncond", "noise", 0.995, 1.0)])
        names = _names(t.tick)
        assert len(names) == 1 and "stage_thresh_kernel_table" in names[0], (count, names)
    # 20 thresholded + 20 plain requests: two runs, one launch of either table family
    cases = thr_requests(40, 2056, 1, sdt, sdt, "uncond", "noise", 0.995, 1.0, thresh=lambda r: r % 2 == 1)
    t, _, _ = check_thresh_table_call(cases, "thresholded beside plain")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [40, 2]
    names = _names(t.tick)
    assert len(names) == 2 and sum("stage_thresh_kernel_table" in n for n in names) == 1 and \
        sum("stage_kernel_table<" in n for n in names) == 1, names
    # two ratios: two groups of thresholded rows, two launches
    cases = thr_requests(6, 2056, 1, sdt, sdt, "uncond", "noise", 0.995, 1.0)
    for r in (1, 4):
        cases[r].st.thr_ratio = 0.5
    cases = [c.on("cpu") for c in cases]
    t, _, _ = check_thresh_table_call(cases, "two ratios")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [6, 2]
    names = _names(t.tick)
    assert len(names) == 2 and all("stage_thresh_kernel_table" in n for n in names), names
    # without the flag the same requests (behind a plain request 0) are launched one by one, as in version 209
    cases = thr_requests(5, 2056, 1, sdt, sdt, "uncond", "noise", 0.995, 1.0, thresh=lambda r: r > 0)
    t = ThreshTableCall([c.on(DEV) for c in cases])
    names = _names(lambda: t.tick(flag=0))
    assert len(names) == 5 and not any("stage_thresh_kernel_table" in n for n in names), names
    assert sum("stage_thresh_kernel<" in n for n in names) == 4, names


@gpu
def test_a_sample_too_large_for_a_row_takes_its_own_launch_in_the_same_call():
    """12296 elements: no row -- the request's clustered launch with its own workspace, beside the others' one table launch"""
    sdt = torch.float16
    cases = thr_requests(5, 2056, 1, sdt, sdt, "uncond", "noise", 0.995, 1.0, seed=2)
    big = thr_requests(3, 12296, 1, sdt, sdt, "uncond", "noise", 0.995, 1.0, seed=2)[2]
    cases.insert(2, big)
    t, _, _ = check_thresh_table_call(cases, "fall back")
    assert t.host[:16].view(torch.int32).tolist()[2:] == [6, 1]
    names = _names(t.tick)
    assert len(names) == 2 and sum("stage_thresh_kernel_table" in n for n in names) == 1, names
