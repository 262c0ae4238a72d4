"""The double-precision sweep (tests/test_gpu_f64_edges.py) without a GPU -- CPU only.

  1. the numpy doubles of every case of the sweep run on CPU arenas and stay inside their payloads;
  2. KD.threshold64 -- the builder's restatement of stage_thresh_kernel_f64 -- against torch.quantile / torch.maximum /
     torch.clamp in float64, bit for bit (a NaN equal to a NaN), on every select-stress pattern, size and ratio;
  3. guarded.F64_BOUND is relative to the largest element: two deliberate mutations of the select -- the order statistic one
     rank off, the lerp weight w replaced by 1 - w -- must each move a stored element by more than the bound, on every
     thresholded input of the sweep whose quantile (not thr_max) decides the threshold;
  4. the coef64 argument of guarded.GuardedLaunch: it survives .on(), the double reads it, a case built without it is what it
     was before the argument existed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as G
import kernel_double as KD
import test_gpu_edges as E
import test_gpu_f64_edges as F
from dpm_solver_amd import _lib as L
from oracle import dpm_oracle as O

F64 = np.float64


# ------------------------------------------------------------------------------------------------
# 1. the doubles of the sweep
# ------------------------------------------------------------------------------------------------
def test_stage_doubles_stay_inside_their_payloads():
    k = 0
    for case in F.a_cases():
        G.run_double(case)
        for name in case.written:
            assert bool(torch.isfinite(case.arenas[name].payload()).all())
        k += 1
    assert k == len(F.a_cells()) * F.PER_CELL


@pytest.mark.parametrize("batch", F.B_BATCHES)
def test_threshold_doubles_stay_inside_their_payloads(batch):
    k = 0
    for case in F.b_cases(batch):
        G.run_double(case)
        for name in case.written:
            assert bool(torch.isfinite(case.arenas[name].payload()).all())
        k += 1
    assert k == len(F.B_SIZES) * F.PER_CELL


def test_select_stress_and_multi_request_doubles_stay_inside_their_payloads():
    for per, name, ratio in F.c_cells():
        case = F.c_case(per, name, ratio)
        assert torch.equal(case.arenas["e0"].payload_bits(), torch.from_numpy(F.c_data(per, name, ratio)).reshape(-1).view(torch.int64))
        F.run_select_double(case)
        assert case.written == {"x_out"}
    for thresh in (True, False):
        for per_request in (True, False):
            cases = F.d_requests(thresh, per_request)
            assert len(cases) == 3 and len({c.req for c in cases}) == 3 and all(c.batch == 3 for c in cases)
            for c in cases:
                G.run_double(c)


# ------------------------------------------------------------------------------------------------
# 2. KD.threshold64 against torch
# ------------------------------------------------------------------------------------------------
def torch_threshold(x0, ratio, max_val):
    """ref :416-425 on a [batch, per] double tensor, with the library the reference calls"""
    t = torch.from_numpy(x0)
    q = torch.quantile(t.abs(), float(ratio), dim=1)
    s = torch.maximum(q, float(max_val) * torch.ones_like(q)).reshape(-1, 1)
    return (torch.clamp(t, -s, s) / s).numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F64).reshape(-1), np.ascontiguousarray(b, dtype=F64).reshape(-1)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("per", F.C_SIZES)
def test_threshold64_is_torch_quantile_bit_for_bit(per):
    for per_, name, ratio in F.c_cells():
        if per_ != per:
            continue
        x0 = F.c_data(per, name, ratio)
        r32, mv = F64(np.float32(ratio)), F64(np.float32(F.PATTERNS[name][1]))      # the record's fp32 scalars, converted exactly
        with np.errstate(all="ignore"):
            got = KD.threshold64(x0, r32, mv)
        d = ~same_bits(got, torch_threshold(x0, r32, mv))
        assert not d.any(), (per, name, ratio, int(np.flatnonzero(d)[0]), int(d.sum()))


# ------------------------------------------------------------------------------------------------
# 3. sensitivity of the bound to a wrong select
# ------------------------------------------------------------------------------------------------
def threshold64_variant(x0, ratio, max_val, rank_off=False, swap_w=False, info=None):
    """KD.threshold64 line by line, with the two seeded defects; info: receives the order statistics and the quantile"""
    rows = x0.reshape(x0.shape[0], -1)
    srt = np.sort(np.abs(rows), axis=1)
    n = rows.shape[1]
    rank = F64(ratio) * F64(n - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    w = rank - F64(lo)
    if info is not None:
        near = sorted({max(lo - 1, 0), lo, hi, min(hi + 1, n - 1)})
        info.update(n=n, lo=lo, hi=hi, w=w, near=srt[:, near])
    if rank_off:                                   # one rank up, or down at the end of the sample
        lo, hi = (lo + 1, hi + 1) if hi + 1 <= n - 1 else (max(lo - 1, 0), max(hi - 1, 0))
    if swap_w:
        w = F64(1.0) - w
    a, b = srt[:, lo], srt[:, hi]
    q = O.fma_rows(w, b - a, a, F64) if w < 0.5 else O.fma_rows(w - F64(1.0), b - a, b, F64)
    q = np.where(np.isnan(rows).any(axis=1), np.nan, q)
    if info is not None and not (rank_off or swap_w):
        info["q"] = q
    s = np.maximum(q, F64(max_val)).reshape((-1,) + (1,) * (x0.ndim - 1))
    with np.errstate(invalid="ignore"):
        return np.minimum(np.maximum(x0, -s), s) / s


def _moved(make, monkeypatch):
    """run the double of the case make() builds as it is and under each seeded defect -> (info, {defect: did a stored element
    move by more than the bound of guarded.verify()?})"""
    info = {}
    with monkeypatch.context() as m, np.errstate(all="ignore"):
        m.setattr(KD, "threshold64", lambda x0, r, mv: threshold64_variant(x0, r, mv, info=info))
        want = make()
        assert G.double_launch(want.st, want.b) == 0
        info["thr_max"] = float(want.coef64.thr_max if want.coef64 is not None else want.st.thr_max)
        out = {}
        for defect in ("rank_off", "swap_w"):
            m.setattr(KD, "threshold64", lambda x0, r, mv, d=defect: threshold64_variant(x0, r, mv, **{d: True}))
            got = make()
            assert G.double_launch(got.st, got.b) == 0
            out[defect] = any(F.differs64(v, F.outputs(want)[k]).any() for k, v in F.outputs(got).items())
    return info, out


def _applies(info):
    """which defects are defects on this input at all: none on a one-element sample (it has one order statistic); the weight
    swap where torch interpolates (lo != hi) with a weight other than one half (1 - w == w there: the same function)"""
    rank_off = info["n"] > 1
    return {"rank_off": rank_off, "swap_w": rank_off and info["lo"] != info["hi"] and info["w"] != 0.5}


def _quantile_decides(info):
    with np.errstate(invalid="ignore"):
        return bool((info["q"] > info["thr_max"]).any())


def test_the_variant_without_a_defect_is_threshold64():
    for per, name, ratio in F.c_cells()[::7]:
        x0 = F.c_data(per, name, ratio)
        with np.errstate(all="ignore"):
            assert same_bits(KD.threshold64(x0, F64(np.float32(ratio)), F64(1.0)), threshold64_variant(x0, F64(np.float32(ratio)), F64(1.0))).all()


@pytest.mark.parametrize("batch", F.B_BATCHES)
def test_a_wrong_select_moves_the_sweeps_outputs_past_the_bound(batch, monkeypatch):
    """every thresholded cell of the sweep whose quantile decides s: no exemption (random data, no ties)"""
    n_checked = 0
    for (per, _), v in F.b_plan(batch):
        make = lambda: F.make_case64("f64-thresh", v, per, batch=batch, seed=per + batch, thresh=True)
        info, moved = _moved(make, monkeypatch)
        assert all(len(set(row)) == len(row) for row in info["near"].tolist())                   # the data has no ties at the rank
        if not _quantile_decides(info):
            continue
        for defect, on in _applies(info).items():
            if on:
                assert moved[defect], (per, batch, v, defect)
                n_checked += 1
    assert n_checked >= len(F.B_SIZES) * 6


def test_a_wrong_select_moves_the_stress_outputs_past_the_bound(monkeypatch):
    """every select-stress input whose quantile decides s.  Exempt: an input of a pattern in F.TIED_BY_CONSTRUCTION where the
    order statistics next to the rank are in fact equal in every sample that decides -- nothing else"""
    n_checked, exempt = 0, set()
    for per, name, ratio in F.c_cells():
        info, moved = _moved(lambda: F.c_case(per, name, ratio), monkeypatch)
        if not _quantile_decides(info):
            continue
        near = info["near"]
        # top55: more than 1024 values in the 256 patterns of one byte -- four or more copies of each, neighbours ONE unit in the
        # last place apart (2^-52 of the value, 45 times below F64_BOUND): no bound relative to the tensor's scale resolves a
        # rank there; test_threshold64_is_torch_quantile_bit_for_bit pins the double on it, bit for bit
        spread = 4 * 2.0 ** -52 if name == "top55" else 0.0
        with np.errstate(invalid="ignore"):
            tied = bool(((np.abs(near - near[:, :1]) <= spread * near[:, :1]) | (near == near[:, :1]) | np.isnan(info["q"])[:, None]
                         | ~(info["q"] > info["thr_max"])[:, None]).all())
        if name in F.TIED_BY_CONSTRUCTION and tied:
            exempt.add(name)
            continue
        for defect, on in _applies(info).items():
            if on:
                assert moved[defect], (per, name, ratio, defect)
                n_checked += 1
    assert exempt <= set(F.TIED_BY_CONSTRUCTION) and n_checked >= 100, (exempt, n_checked)
    for name in ("top22", "top33", "top44", "subnormal", "last_in_bin", "nan", "neg_inf"):      # never exempt
        assert name not in F.TIED_BY_CONSTRUCTION


# ------------------------------------------------------------------------------------------------
# 4. guarded.GuardedLaunch(coef64=...)
# ------------------------------------------------------------------------------------------------
def test_coef64_survives_on_and_like_and_the_double_reads_it():
    v = F._plain_variant(form="MS3", guidance="classifier-free", coef64=True, blend="pack")
    case = F.make_case64("f64", v, 768, seed=9)
    assert case.coef64 is not None and C.addressof(case.b.coef64.contents) == C.addressof(case.coef64)
    twin = case.on("cpu")
    assert twin.coef64 is case.coef64 and C.addressof(twin.b.coef64.contents) == C.addressof(case.coef64)
    third = G.GuardedLaunch(case.family, case.st, case.n, case.sd, case.ed, like=case, **case.kw)
    assert third.coef64 is case.coef64 and bool(third.b.coef64)
    for f in ("alpha_e", "sigma_e", "cfg_scale", "cx", "c0", "c1", "c2", "blend_alpha", "blend_sigma"):
        d = float(getattr(case.coef64, f))
        assert float(np.float32(d)) != d, f                      # no fp32 number: the fp32 record cannot stand in for it
    assert abs(case.coef64.sigma_e ** 2 + case.coef64.alpha_e ** 2 - 1.0) < 1e-15
    want = G.run_double(case)
    plain = G.run_double(F.make_case64("f64", dict(v, coef64=False), 768, seed=9))
    assert not bool(plain.b.coef64) and plain.coef64 is None
    for k in ("x_out", "m_out"):                                 # the same data under the fp32 record misses the bound
        assert torch.equal(want.pristine["x"], plain.pristine["x"])
        assert F.differs64(F.outputs(plain)[k], F.outputs(want)[k]).any(), k
    twin_out = G.run_double(twin)
    twin_out.verify(want)


def test_a_case_without_coef64_is_what_it_was():
    """the record, the keyword set .on() forwards and the data of a case built without the argument"""
    c = E.make_case("f64", E.VARIANTS["f64"][4], 513, torch.float64, torch.float64, seed=2)
    assert c.coef64 is None and not bool(c.b.coef64) and "coef64" not in c.kw
    assert sorted(c.kw) == ["batch", "blend", "dup", "noise_seed", "offset", "per_request_stages", "req", "seed", "sep_xe", "stride", "ws_bytes"]
    d = c.on("cpu")
    assert d.coef64 is None and not bool(d.b.coef64)
    b0, b1 = L.Buffers(), c.b
    for k, a in c.arenas.items():
        if k in G.INPUTS or k in c.named:
            setattr(b0, k, a.ptr)
    b0.n, b0.batch, b0.state_dtype, b0.eps_dtype, b0.eps_stride, b0.opts = c.n, c.batch, L.DTYPE_F64, L.DTYPE_F64, 0, b1.opts
    assert bytes(b0) == bytes(b1)
