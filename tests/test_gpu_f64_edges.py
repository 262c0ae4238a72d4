"""Guard-banded sweep of the double-precision unit (csrc/dpm_f64.hip) through the C ABI, at sizes taken from ITS constants:
stage_kernel_f64 owns U64 x 256 = 512 elements per workgroup in two 256-element rows; stage_thresh_kernel_f64 is one
1024-thread workgroup per sample that selects among at most CAP64 = 1024 candidates in LDS, reads UT64 = 4 rows per select
iteration and stores UF64 = 2 rows per store iteration; add_noise_kernel_f64 / blend_kernel_f64 are grid-stride loops capped
at 16 workgroups per CU.  Every launch runs on operands between guards (tests/guarded.py), float64 state and outputs, after
its numpy double on the CPU copy of the same case, and is followed by verify(): guards, inputs, the outputs a stage must not
write, no payload element skipped, values within guarded.F64_BOUND of the double.  Which variant every cell runs is a table
(`variants`); test_tables_meet_the_coverage_rule asserts the rule on it.  tests/test_f64_edges_host.py runs the doubles of
every case here without a GPU, ties KD.threshold64 to torch.quantile and shows that F64_BOUND cannot hide a wrong select.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C
import math
import random
import time
import types

import numpy as np
import pytest
import torch

import guarded as G
import kernel_double as KD
import test_gpu_edges as E
from dpm_solver_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64

# ---- the constants of csrc/dpm_f64.hip the sizes below are taken from
ROW64, U64 = 256, 2                      # stage_kernel_f64: lanes per workgroup, rows per workgroup
T64, CAP64, UT64, UF64 = 1024, 1024, 4, 2  # stage_thresh_kernel_f64: lanes, candidate list, rows per select / store iteration
GRID_CAP_PER_CU = 16                     # add_noise_kernel_f64 / blend_kernel_f64: workgroups per CU at most

A_SIZES = [1, ROW64 - 1, ROW64, ROW64 + 1, U64 * ROW64 - 1, U64 * ROW64, U64 * ROW64 + 1, 3 * ROW64 - 1, 3 * ROW64, 3 * ROW64 + 1,
           2 * U64 * ROW64, 2 * U64 * ROW64 + 1, 3 * U64 * ROW64 + 1]
A_OFFSET1 = [ROW64 + 1, 2 * U64 * ROW64 + 1]            # ... that also run one element (8 bytes) past the 16-byte boundary
B_SIZES = [1, 2, CAP64 - 1, CAP64, CAP64 + 1, UF64 * T64 - 1, UF64 * T64, UF64 * T64 + 1, UT64 * T64 - 1, UT64 * T64, UT64 * T64 + 1,
           6145]
B_BATCHES = (1, 3)
C_SIZES = [CAP64 + 1, UT64 * T64 + 1, 6145]
C_BATCH = 3
RATIOS = [0.995, 0.5, 1.0, 0.0, 1.0 / 3.0]
THR_MAX = [1.0, 1e-3]
PER_CELL = 12                            # variants per cell: a multiple of every axis' length but thr_ratio's (5 <= 12)

# ---- the variant axes; every cell meets every value of every axis (test_tables_meet_the_coverage_rule)
AXES = {
    "form": ["LIN1", "TWO", "TWO_BASE", "MS3", "SS3T", "DENOISE"],           # TWO_BASE: TWO with DPM_F_BASE_HIST; SS3T: separate xe
    "model": ["noise", "x_start", "v", "score"],
    "to_x0": [True, False],
    "guidance": ["uncond", "classifier-free", "classifier"],
    "store_m": [True, False],
    "dup": [True, False],                                                      # x_out2 named or not
    "stride_batch": [0, 2, 3],                                                 # dense | eps_stride = 2 x per with that batch
    "blend": [None, "pack", "ragged", "no_b"],                                 # no_b: the pack period without blend_b
    "coef64": [True, False],
}
THR_AXES = dict({k: v for k, v in AXES.items() if k != "stride_batch"}, stride=[False, True], thr_ratio=RATIOS, thr_max=THR_MAX)


def a_cells():
    return [(n, 0) for n in A_SIZES] + [(n, 1) for n in A_OFFSET1]


def variants(axes, key):
    """PER_CELL variants of one cell: every axis deals its values round the slots in an order of its own (fixed seed per cell),
    so that every value of every axis is met in every cell and no two axes are tied to each other"""
    rng = random.Random(key)
    out = [dict() for _ in range(PER_CELL)]
    for name, vals in axes.items():
        slots, r = list(range(PER_CELL)), rng.randrange(len(vals))
        rng.shuffle(slots)
        for i, s in enumerate(slots):
            out[s][name] = vals[(i + r) % len(vals)]
    return out


def a_plan():
    return [((n, off), v) for n, off in a_cells() for v in variants(AXES, 7919 * n + off)]


def b_plan(batch):
    return [((per, batch), v) for per in B_SIZES for v in variants(THR_AXES, 104729 * per + batch)]


def _odd_divisor(n):
    return next((q for q in range(3, n, 2) if n % q == 0), None)


def blend_of(v, n):
    """(mask_period, with blend_b) at n elements -- pack / no_b: 8 where 8 divides n; else (and ragged) the smallest odd divisor of
    n; else n itself, a mask as long as the state"""
    if not v["blend"]:
        return None
    if v["blend"] != "ragged" and n % 8 == 0 and n > 8:
        return 8, v["blend"] != "no_b"
    return _odd_divisor(n) or n, v["blend"] != "no_b"


def _met(axes, vs, n_of):
    """assert that the variants `vs` of a cell meet every value of every axis (the blend periods as far as n has them)"""
    for name, vals in axes.items():
        assert {v[name] for v in vs} == set(vals), name
    periods = [(blend_of(v, n_of(v)), n_of(v)) for v in vs if v["blend"]]
    assert {b[1] for b, _ in periods} == {True, False}
    for (p, _), n in periods:
        assert n % p == 0 and 1 <= p <= n
    assert any(p == 8 for (p, _), n in periods) or all(n % 8 for _, n in periods)             # period 8 wherever 8 divides n
    assert any(p < n for (p, _), n in periods) or not any(_odd_divisor(n) for _, n in periods)  # a broadcast mask wherever n has one


def test_tables_meet_the_coverage_rule():
    assert (ROW64, U64, T64, CAP64, UT64, UF64) == (256, 2, 1024, 1024, 4, 2) and G.GUARD >= UT64 * T64
    assert A_SIZES == [1, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1024, 1025, 1537]
    assert len(A_OFFSET1) == 2 and set(A_OFFSET1) <= set(A_SIZES)
    assert B_SIZES == [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6145] and B_BATCHES == (1, 3)
    assert C_SIZES == [1025, 4097, 6145] and C_BATCH == 3
    assert RATIOS == [0.995, 0.5, 1.0, 0.0, 1.0 / 3.0] and THR_MAX == [1.0, 1e-3]
    assert AXES == {"form": ["LIN1", "TWO", "TWO_BASE", "MS3", "SS3T", "DENOISE"], "model": ["noise", "x_start", "v", "score"],
                    "to_x0": [True, False], "guidance": ["uncond", "classifier-free", "classifier"], "store_m": [True, False],
                    "dup": [True, False], "stride_batch": [0, 2, 3], "blend": [None, "pack", "ragged", "no_b"],
                    "coef64": [True, False]}
    assert set(THR_AXES) == (set(AXES) - {"stride_batch"}) | {"stride", "thr_ratio", "thr_max"}
    assert THR_AXES["stride"] == [False, True] and THR_AXES["thr_ratio"] is RATIOS and THR_AXES["thr_max"] is THR_MAX
    assert all(PER_CELL >= len(v) for v in THR_AXES.values()) and all(PER_CELL % len(v) == 0 for v in AXES.values())
    pa = a_plan()
    assert {c for c, _ in pa} == set(a_cells()) and {n for n, o in a_cells() if o == 0} == set(A_SIZES)
    for cell in a_cells():
        _met(AXES, [v for c, v in pa if c == cell], lambda v: cell[0] * (v["stride_batch"] or 1))
    for batch in B_BATCHES:
        pb = b_plan(batch)
        assert {c for c, _ in pb} == {(per, batch) for per in B_SIZES}
        for per in B_SIZES:
            _met(THR_AXES, [v for c, v in pb if c == (per, batch)], lambda v: per * batch)
    # the select stress: every pattern at every size and ratio; the names the sensitivity check may exempt are patterns
    assert {(per, name, r) for per, name, r in c_cells()} == {(per, name, r) for per in C_SIZES for name in PATTERNS for r in RATIOS}
    assert set(TIED_BY_CONSTRUCTION) <= set(PATTERNS)
    assert {"top22", "top33", "top44", "top55", "ties", "constant", "two_values", "zeros", "subnormal", "last_in_bin", "nan",
            "inf_at", "inf_next", "inf_above", "neg_inf"} == set(PATTERNS)


# ------------------------------------------------------------------------------------------------
# stage records, coef64 records, cases
# ------------------------------------------------------------------------------------------------
def make_stage64(v, seed, thresh=False):
    form = "TWO" if v["form"] == "TWO_BASE" else v["form"]
    st = E.make_stage(form, v["guidance"], v["model"], v["store_m"], thresh=thresh, blend=bool(v["blend"]), seed=seed)
    st.flags &= ~(L.F_TO_X0 | L.F_BASE_HIST)
    st.flags |= (L.F_TO_X0 if v["to_x0"] else 0) | (L.F_BASE_HIST if v["form"] == "TWO_BASE" else 0)
    if thresh:
        st.thr_ratio, st.thr_max = v["thr_ratio"], v["thr_max"]
    return st


def coef64_of(st):
    """the dpm_stage_f64 record beside `st`: every scalar the fp32 value times (1 + 2^-30) -- no fp32 number, so a kernel that
    read the fp32 record instead misses F64_BOUND --, sigma_e = sqrt(1 - alpha_e^2) evaluated in double, thr_ratio kept in [0, 1]"""
    c, up = L.StageF64(), 1.0 + 2.0 ** -30
    for f in ("alpha_e", "cfg_scale", "cg_scale", "cx", "c0", "c1", "c2", "thr_max", "blend_alpha", "blend_sigma"):
        setattr(c, f, float(getattr(st, f)) * up)
    c.sigma_e = math.sqrt(1.0 - c.alpha_e ** 2)
    for j in range(5):
        c.k[j] = float(st.k[j]) * up
    c.thr_ratio = min(1.0, float(st.thr_ratio) * up)
    return c


def make_case64(family, v, size, batch=1, offset=0, seed=0, req=0, thresh=False, per_request=False):
    """the CPU GuardedLaunch of variant v: `size` elements per sample (a strided or thresholded cell), else in all"""
    st = make_stage64(v, seed * 131 + (req if per_request else 0), thresh)
    if thresh:
        stride = 2 * size if v["stride"] else 0
    else:
        batch, stride = (v["stride_batch"] or 1), (2 * size if v["stride_batch"] else 0)
    n, kw = size * batch, {}
    if v["blend"]:
        kw["blend"] = blend_of(v, n)
    return G.GuardedLaunch(family, st, n, F64, F64, batch=batch, offset=offset, dup=v["dup"], stride=stride,
                           sep_xe=v["form"] == "SS3T", seed=seed, req=req, per_request_stages=per_request,
                           coef64=coef64_of(st) if v["coef64"] else None, **kw)


def a_cases():
    for (n, off), v in a_plan():
        yield make_case64("f64", v, n, offset=off, seed=n + 7 * off)


def b_cases(batch):
    for (per, _), v in b_plan(batch):
        yield make_case64("f64-thresh", v, per, batch=batch, seed=per + batch, thresh=True)


# ------------------------------------------------------------------------------------------------
# (c) select stress: the record dynamic_thresholding_fn builds, e0 owned by the test
# ------------------------------------------------------------------------------------------------
def rank_of(per, ratio):
    """(lo, hi) of torch.quantile's rank as the launcher and the double compute it: the record's fp32 ratio times (per - 1), in double"""
    rank = np.float64(np.float32(ratio)) * np.float64(per - 1)
    return int(np.floor(rank)), int(np.ceil(rank))


def _shared_top(t):
    """every value of a sample shares its top t pattern bits (11 exponent bits, t - 11 mantissa bits): 1.x + k * 2^-52 * step
    with k below the number of distinct values the low 63 - t bits hold, evenly spaced, shuffled, signs mixed"""
    def build(per, ratio, rng):
        low, (lo, hi) = 63 - t, rank_of(per, ratio)
        out = np.empty((C_BATCH, per))
        for j in range(C_BATCH):
            r = np.arange(per, dtype=np.int64)
            if per <= 1 << low:     # distinct; an eighth of the range is left out below rank lo, above it and above rank hi,
                # so that neither a rank one off nor a swapped weight hides below F64_BOUND where the steps are a few ulps
                k = r * (((1 << low) // 2) // per) + ((1 << low) // 8) * ((r >= lo).astype(np.int64) + (r > lo) + (r > hi))
            else:                   # more values than patterns: ties, one unit in the last place apart
                k = r % (1 << low)
            k = k.astype(np.uint64)
            bits = np.uint64(0x3FF0000000000000) | (np.uint64(j + 1) << np.uint64(low)) | k
            assert bool((k < (1 << low)).all())
            out[j] = rng.permutation(bits.view(np.float64)) * rng.choice([-1.0, 1.0], per)
        return out
    return build


def _ties(per, ratio, rng):
    """more copies of 1.5 than the candidate list holds, three values below and the rest above; where the rank allows it the
    copies END at rank lo, so that the next order statistic is the smallest value above them"""
    lo, _ = rank_of(per, ratio)
    copies = lo - 2 if lo - 2 > CAP64 and per - lo - 1 >= 1 else per - 6
    out = np.empty((C_BATCH, per))
    for j in range(C_BATCH):
        above = 1.6 + np.arange(per - 3 - copies) * 0.25
        row = np.concatenate([[0.5, -0.7, 1.2], np.full(copies, 1.5), above])
        out[j] = rng.permutation(row) * (1.0 + j)
    return out


def _constant(per, ratio, rng):
    return np.stack([np.full(per, c) for c in (1.25, -1.25, 3.0)])


def _two_values(per, ratio, rng):
    return np.where(rng.random((C_BATCH, per)) < 0.3, 3.0, -0.5)


def _zeros(per, ratio, rng):
    z = np.where(rng.random((C_BATCH, per)) < 0.5, 0.0, -0.0)
    return np.where(rng.random((C_BATCH, per)) < 0.75, z, rng.standard_normal((C_BATCH, per)) * 2.0)


def _subnormal(per, ratio, rng):
    return rng.standard_normal((C_BATCH, per)) * 1e-310


def _last_in_bin(per, ratio, rng):
    """ranks 0 .. lo lie in [1, 1 + 2^-7), 2^-20 apart (the bins of the second histogram pass are 2^-11 wide), the rest in
    [2, 4): the wanted value is the largest member of every bin it falls in, the next order statistic has another exponent"""
    lo, _ = rank_of(per, ratio)
    row = np.concatenate([1.0 + np.arange(lo + 1) * 2.0 ** -20, 2.0 + np.arange(per - lo - 1) * 2.0 ** -13])
    return np.stack([rng.permutation(row) * rng.choice([-1.0, 1.0], per) * 2.0 ** j for j in range(C_BATCH)])


def _nan(per, ratio, rng):
    out = rng.standard_normal((C_BATCH, per)) * 2.0
    out[1, per // 3] = np.nan
    return out


def _inf(first):
    """+inf from ascending rank first(lo, hi) on (signs mixed below it)"""
    def build(per, ratio, rng):
        lo, hi = rank_of(per, ratio)
        out = rng.standard_normal((C_BATCH, per)) * 2.0
        for j in range(C_BATCH):
            order = np.argsort(np.abs(out[j]))
            out[j, order[min(first(lo, hi), per):]] = np.inf
        return out
    return build


def _neg_inf(per, ratio, rng):
    out = rng.standard_normal((C_BATCH, per)) * 2.0
    out[:, per // 2] = -np.inf
    return out


# name -> (builder, thr_max of the record)
PATTERNS = {"top22": (_shared_top(22), 1.0), "top33": (_shared_top(33), 1.0), "top44": (_shared_top(44), 1.0),
            "top55": (_shared_top(55), 1.0), "ties": (_ties, 1.0), "constant": (_constant, 1.0), "two_values": (_two_values, 1.0),
            "zeros": (_zeros, 1.0), "subnormal": (_subnormal, 0.0), "last_in_bin": (_last_in_bin, 1.0), "nan": (_nan, 1.0),
            "inf_at": (_inf(lambda lo, hi: lo), 1.0), "inf_next": (_inf(lambda lo, hi: lo + 1), 1.0),
            "inf_above": (_inf(lambda lo, hi: hi + 1), 1.0), "neg_inf": (_neg_inf, 1.0)}
# the patterns whose neighbouring order statistics may be equal BY CONSTRUCTION (tests/test_f64_edges_host.py: an input of one
# of these is exempt from the sensitivity check only where they are in fact equal in every sample)
TIED_BY_CONSTRUCTION = ("top55", "ties", "constant", "two_values", "zeros", "inf_at", "inf_next", "inf_above")


def c_cells():
    return [(per, name, r) for per in C_SIZES for name in PATTERNS for r in RATIOS]


def c_data(per, name, ratio):
    rng = np.random.default_rng([per, sorted(PATTERNS).index(name), RATIOS.index(ratio)])
    out = np.ascontiguousarray(PATTERNS[name][0](per, ratio, rng), dtype=np.float64)
    assert out.shape == (C_BATCH, per)
    return out


def c_case(per, name, ratio):
    """DENOISE + DPM_F_THRESH, noise network, no conversion: the model value is e0 bit for bit"""
    st = L.Stage()
    st.h1_slot = st.h2_slot = st.m_slot = -1
    st.form, st.flags = L.FORM_DENOISE, L.F_THRESH
    st.thr_ratio, st.thr_max = ratio, PATTERNS[name][1]
    st.alpha_e, st.sigma_e, st.cfg_scale = 1.0, 0.0, 1.0
    e0 = torch.from_numpy(c_data(per, name, ratio)).reshape(-1)
    data = types.SimpleNamespace(pristine={"x": torch.zeros(per * C_BATCH, dtype=F64).view(torch.int64), "e0": e0.view(torch.int64)},
                                 coef64=None)
    return G.GuardedLaunch("f64-select:%s:%g" % (name, ratio), st, per * C_BATCH, F64, F64, batch=C_BATCH, like=data)


def run_select_double(case):
    """G.run_double for a select-stress case (the infinities of a pattern meet inf - inf in the lerp, as they do in torch's)"""
    with np.errstate(invalid="ignore"):
        return G.run_double(case)


def differs64(got, want):
    """the mask of guarded.verify() for double states -- beyond F64_BOUND of the largest wanted magnitude -- with a NaN equal to
    a NaN and an infinity equal to itself (the largest FINITE wanted magnitude sets the bound)"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    fin = np.isfinite(want)
    bound = G.F64_BOUND * (float(np.abs(want[fin]).max()) if fin.any() else 0.0)
    with np.errstate(invalid="ignore"):
        near = np.abs(got - want) <= bound
    same = (np.isnan(got) & np.isnan(want)) | (~fin & (got == want))
    return ~np.where(fin, near, same)


def outputs(case):
    return {k: case.arenas[k].payload().numpy() for k in sorted(case.written)}


def verify_nan_aware(dev, want):
    """verify() where the wanted values hold NaNs or infinities: its structure checks, then differs64 on every written output"""
    dev.verify()
    for k, w in outputs(want).items():
        d = differs64(outputs(dev)[k], w)
        assert not d.any(), (dev.family, k, int(np.flatnonzero(d)[0]), int(d.sum()))


# ------------------------------------------------------------------------------------------------
# (d) multi-request calls
# ------------------------------------------------------------------------------------------------
def d_requests(thresh, per_request):
    """three double requests: thresholded at CAP64 + 1 per sample (batch 3), or plain at one element past a workgroup's tile"""
    size = CAP64 + 1 if thresh else U64 * ROW64 + 1
    vs = variants(THR_AXES if thresh else AXES, 31 + thresh)
    vs = [dict(v, stride_batch=3) for v in vs]                   # (batch 3 in the plain calls too, eps_stride = 2 x per)
    return [make_case64("f64-multi", vs[r] if per_request else vs[0], size, batch=3, seed=size, req=r, thresh=thresh,
                        per_request=per_request) for r in range(3)]


# ------------------------------------------------------------------------------------------------
# the GPU tests
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    yield DEV
    torch.cuda.synchronize()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(case):
    rc = L.lib.dpm_stage_launch(C.byref(case.st), C.byref(case.b), _stream())
    torch.cuda.synchronize()
    return rc


@gpu
def test_stage_kernel_f64(dev):
    t0, k = time.time(), 0
    for case in a_cases():
        E.run_single(case)
        k += 1
    assert k == len(a_cells()) * PER_CELL
    print("stage_kernel_f64: %d launches in %.2f s" % (k, time.time() - t0))


@gpu
@pytest.mark.parametrize("batch", B_BATCHES)
def test_stage_thresh_kernel_f64(batch, dev):
    """no variant is refused: the double unit takes thresholding together with the blend epilogue, eps_stride, x_out2 and every
    guidance kind -- a refusal would have to write nothing"""
    t0, k = time.time(), 0
    for case in b_cases(batch):
        want, d = G.run_double(case), case.on(dev)
        rc = _launch(d)
        assert rc == 0, (rc, L.lib.dpm_last_error())
        d.verify(want, rc)
        k += 1
    assert k == len(B_SIZES) * PER_CELL
    print("stage_thresh_kernel_f64 batch %d: %d launches in %.2f s" % (batch, k, time.time() - t0))


@gpu
@pytest.mark.parametrize("per", C_SIZES)
def test_select_stress(per, dev):
    t0 = time.time()
    for per_, name, ratio in c_cells():
        if per_ != per:
            continue
        case = run_select_double(c_case(per, name, ratio))
        d = case.on(dev)
        rc = _launch(d)
        assert rc == 0, (rc, L.lib.dpm_last_error())
        verify_nan_aware(d, case)
        if name == "nan":                        # that sample is all NaN, its neighbours are not touched by it
            y = outputs(d)["x_out"].reshape(C_BATCH, per)
            assert np.isnan(y[1]).all() and np.isfinite(y[0]).all() and np.isfinite(y[2]).all()
    print("select stress per %d: %.2f s" % (per, time.time() - t0))


@gpu
@pytest.mark.parametrize("per_request", [False, True], ids=["one-stage", "per-request-stages"])
@pytest.mark.parametrize("thresh", [True, False], ids=["thresh-1025", "plain-513"])
def test_multi_request_calls(thresh, per_request, dev):
    """no fused double kernel: dpm_stage_launch_multi launches the requests one by one -- each matches its double and, bit for
    bit, its own lone launch"""
    cases = d_requests(thresh, per_request)
    wants, devs, lone = [G.run_double(c) for c in cases], [c.on(dev) for c in cases], [c.on(dev) for c in cases]
    arr_b = (L.Buffers * 3)(*[d.b for d in devs])
    st = (L.Stage * 3)(*[d.st for d in devs]) if per_request else C.byref(devs[0].st)
    rc = L.lib.dpm_stage_launch_multi(st, arr_b, 3, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants)
    for d, l in zip(devs, lone):
        assert _launch(l) == 0
        for k in sorted(d.written):
            assert torch.equal(d.arenas[k].payload_bits().cpu(), l.arenas[k].payload_bits().cpu()), (d.req, k)


def _plain_variant(**kw):
    return dict(dict(form="TWO", model="noise", to_x0=True, guidance="uncond", store_m=True, dup=False, stride_batch=0, blend=None,
                     coef64=False), **kw)


def _refused(d, code, text, launch=_launch):
    rc = launch(d)
    assert rc == code and text in L.lib.dpm_last_error(), (rc, L.lib.dpm_last_error())
    d.verify(rc=rc)


@gpu
def test_errors_write_nothing(dev):
    n = U64 * ROW64 + 1
    v = _plain_variant()
    mk = lambda st, sd=F64, ed=F64, **kw: G.GuardedLaunch("f64-error", st, n, sd, ed, seed=3, **kw).on(dev)
    _refused(mk(make_stage64(v, 1), ed=torch.float32), L.ERR_UNSUPPORTED, b"a double state needs double network outputs")
    _refused(mk(make_stage64(v, 1), sd=torch.float32), L.ERR_UNSUPPORTED, b"a double state needs double network outputs")
    st = make_stage64(v, 2)
    st.flags |= L.F_NOISE
    _refused(mk(st, noise_seed=5), L.ERR_ARG, b"DPM_F_NOISE with a double state")
    _refused(mk(E.make_stage("UNIPC", seed=3)), L.ERR_UNSUPPORTED, b"DPM_FORM_UNIPC with a double state")
    for flag, name in ((L.F_CFG_RESCALE, b"DPM_F_CFG_RESCALE"), (L.F_CFG_APG, b"DPM_F_CFG_APG"), (L.F_CFG_ZSTAR, b"DPM_F_CFG_ZSTAR")):
        st = make_stage64(_plain_variant(guidance="classifier-free"), 4)
        st.flags |= flag
        st.thr_max = 0.0                          # (the momentum of DPM_F_CFG_APG: none)
        _refused(mk(st, batch=1), L.ERR_UNSUPPORTED, name + b" with a double state")
    # device-resident coefficients: dpm_adaptive_stage_launch on a double state
    import test_gpu_adaptive_kernels as AK
    hd, tmpl, recs = AK.stage_handle(2, "dpmsolver", "uncond", "noise")
    d = mk(recs[0], sep_xe=recs[0].xe_src == L.SRC_TMP)
    _refused(d, L.ERR_UNSUPPORTED, b"device-resident coefficients with a double state",
             launch=lambda c: (L.lib.dpm_adaptive_stage_launch(hd.h, 0, C.byref(tmpl[0]), C.byref(c.b), _stream()),
                               torch.cuda.synchronize())[0])
    # a pointer 4 bytes past an 8-byte boundary: an input, an output
    for field in ("e0", "h1", "x_out", "m_out"):
        d = mk(make_stage64(v, 5))
        setattr(d.b, field, getattr(d.b, field) + 4)
        _refused(d, L.ERR_ALIGN, b"not 8-byte aligned")


def _device_cap():
    n_cu, lds = C.c_int(), C.c_int()
    L.check(L.lib.dpm_device_info(C.byref(n_cu), C.byref(lds), C.create_string_buffer(64), 64))
    assert n_cu.value == torch.cuda.get_device_properties(0).multi_processor_count
    return n_cu.value * GRID_CAP_PER_CU


def _arena(values, device):
    t = torch.as_tensor(values, dtype=F64).reshape(-1)
    return G.Arena(F64, t.numel(), device, bits=t.view(torch.int64))


def _written_between_guards(out, what):
    out.verify(what, out.payload_bits())                                     # both guards as they were
    assert not bool((out.payload_bits() == G.FILL[8]).any()), what + ": a payload element was not stored"
    return out.payload()


F_SIZES = lambda cap: [1, ROW64 + 1, cap * 256 + 257]                        # the last: the grid-stride loop goes round twice, ragged


@gpu
@pytest.mark.parametrize("ns_dtype", [torch.float64, torch.float32], ids=["f64-schedule", "f32-schedule"])
def test_add_noise_f64_past_the_grid_cap(ns_dtype, dev):
    import dpm_solver_amd as D
    ns = D.NoiseScheduleVP("discrete", betas=torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64), dtype=ns_dtype)
    cap, nt = _device_cap(), 2
    for n in F_SIZES(cap):
        g = torch.Generator().manual_seed(n)
        xs, nz = torch.randn(n, dtype=F64, generator=g) * 1.7, torch.randn(nt * n, dtype=F64, generator=g)
        for entry in ("dpm_add_noise_launch", "dpm_add_noise_launch_f64"):
            x, noise, out = _arena(xs, dev), _arena(nz, dev), G.Arena(F64, nt * n, dev)
            if entry == "dpm_add_noise_launch":
                tt = torch.tensor([0.3, 0.9])                               # fp32 times, as DPM_Solver.add_noise passes them
                th = tt.numpy()
                rc = L.lib.dpm_add_noise_launch(ns._h, th.ctypes.data_as(C.POINTER(C.c_float)), nt, x.ptr, noise.ptr, out.ptr, n,
                                                L.DTYPE_F64, _stream())
            else:
                tt = torch.tensor([0.3, 0.9], dtype=F64)
                th = tt.numpy()
                rc = L.lib.dpm_add_noise_launch_f64(ns._h, th.ctypes.data_as(C.POINTER(C.c_double)), nt, x.ptr, noise.ptr, out.ptr, n,
                                                    _stream())
            torch.cuda.synchronize()
            assert rc == 0, (rc, L.lib.dpm_last_error())
            x.verify("x"), noise.verify("noise")
            got = _written_between_guards(out, "%s n=%d" % (entry, n)).reshape(nt, n)
            a, sg = ns.marginal_alpha(tt).double().reshape(nt, 1), ns.marginal_std(tt).double().reshape(nt, 1)
            want = a * xs + sg * nz.reshape(nt, n)
            assert float((got - want).abs().max()) <= 1e-15 * float(want.abs().max()), (entry, n)


def blend64(x, mask, a, b, alpha, sigma):
    """the numpy double of blend_kernel_f64 (the double branch of KD.launch_raw_double's epilogue): x m + (1 - m) (alpha a + sigma b)"""
    m = mask[np.arange(x.size) % mask.size]
    r = a if b is None else np.float64(alpha) * a + np.float64(sigma) * b
    return x * m + (np.float64(1.0) - m) * r


@gpu
def test_blend_f64_past_the_grid_cap(dev):
    cap = _device_cap()
    alpha, sigma = float(np.float32(0.8)), float(np.float32(0.6))
    for n in F_SIZES(cap):
        rng = np.random.default_rng(n)
        xs, av, bv = (rng.standard_normal(n) for _ in range(3))
        for period in (8, 7, n):
            mk = rng.random(period)
            for with_b in (True, False):
                x, mask, a, b, out = _arena(xs, dev), _arena(mk, dev), _arena(av, dev), _arena(bv, dev), G.Arena(F64, n, dev)
                rc = L.lib.dpm_blend_launch(x.ptr, mask.ptr, a.ptr, b.ptr if with_b else None, alpha, sigma, out.ptr, n, period,
                                            L.DTYPE_F64, _stream())
                torch.cuda.synchronize()
                assert rc == 0, (rc, L.lib.dpm_last_error())
                for name, ar in (("x", x), ("mask", mask), ("a", a), ("b", b)):
                    ar.verify(name)
                got = _written_between_guards(out, "blend n=%d period=%d" % (n, period)).numpy()
                want = blend64(xs, mk, av, bv if with_b else None, alpha, sigma)
                assert float(np.abs(got - want).max()) <= G.F64_BOUND * float(np.abs(want).max()), (n, period, with_b)


@gpu
@pytest.mark.parametrize("ns_dtype", [torch.float64, torch.float32], ids=["f64-schedule", "f32-schedule"])
def test_thresholded_cfg_run_end_to_end(ns_dtype, dev, monkeypatch):
    """sample(x.double()) with dynamic thresholding under classifier-free guidance at 1728 elements per sample -- a histogram
    pass under the real plan and its coef64 records -- against the numpy double on the CPU, at the bound of
    test_gpu_parity.py::test_double_precision_state_on_the_gpu"""
    import dpm_solver_amd as D
    import dpm_solver_amd.solver as S
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64)
    xc = torch.from_numpy(np.random.default_rng(65).standard_normal((3, 3, 24, 24)))
    assert xc[0].numel() == 1728 > CAP64
    cond = torch.arange(1, 4, dtype=torch.float64) * 0.5
    net = lambda xx, t: xx * 0.5 * torch.cos(t.to(xx.dtype) * 1e-3).reshape(-1, 1, 1, 1) + 0.1
    netc = lambda xx, t, c: net(xx, t) * (1.0 + 0.1 * c.to(xx.dtype).reshape(-1, 1, 1, 1))

    def solver(device):
        ns = D.NoiseScheduleVP("discrete", betas=betas, dtype=ns_dtype)
        fn = D.model_wrapper(netc, ns, guidance_type="classifier-free", condition=cond.to(device),
                             unconditional_condition=torch.zeros(3, dtype=torch.float64, device=device), guidance_scale=3.0)
        return D.DPM_Solver(fn, ns, correcting_x0_fn="dynamic_thresholding")
    got = solver(dev).sample(xc.to(dev), steps=6, order=2)
    with monkeypatch.context() as m:
        KD.install_cpu_double(m, S, D)
        want = solver("cpu").sample(xc, steps=6, order=2)
    assert got.dtype == torch.float64 and got.is_cuda
    assert float((got.cpu() - want).abs().max()) <= 1e-14 * float(want.abs().max())
