"""The kernels of the device-side adaptive solver (dpm_adaptive_*, csrc/dpm_kernels.hip) one by one through the C ABI, on
operands between guard bands (tests/guarded.py), against the numpy restatements of tests/adaptive_double.py:

  (a) the error norm -- dpm_adaptive_error with G workgroups per sample (chunk rounding, ragged last chunk, vector and
      one-element-per-lane route at G > 1, scratch regrow, counters) and the host loop's dpm_adaptive_error_launch;
  (b) the commit of dpm_adaptive_begin -- vector and scalar route, past the grid cap, and the begins that must write nothing;
  (c) the controller -- scripted error estimates, every status word, the ring of 32 verdicts, the time vectors;
  (d) dpm_adaptive_stage_launch -- the kernels that read their coefficients from device memory;
  and a NaN estimate, which ends a run with the verdict 2.

tests/test_adaptive_double_host.py shows without a GPU that the restatements are right and that every comparison used here
rejects a defective kernel.  Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adaptive_double as AD
import dpm_solver_amd as D
import guarded as G
from dpm_solver_amd import _lib as L
from engine_cases import make_schedule
from test_adaptive_double_host import ATOL, RTOL, desc_of
from test_gpu_edges import OFFSET1, SIZES

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
PER_SAMPLE = [1, 7, 8, 9, 255, 2048, 8191, 16383, 16384, 16385, 16392, 24584, 65544, 524288, 532480]
BATCHES = [1, 2, 3, 17, 600]
MAX_ELEMS = 4 << 20                               # cells above that are dropped ...
FORCED_G1 = (600, 16384)                          # ... but this one: a sample that could be split, a batch that forbids it
ERR_OFFSET1 = [2048, 16392, 65544]                # also one element past the 16-byte boundary (the scalar route)
ALGO_OF = {"sd": "dpmsolver++", "vp_linear": "dpmsolver", "cosine1000": "dpmsolver++"}


def error_cells():
    """(batch, per_sample, offset) of every error-norm launch"""
    out = [(b, p, 0) for p in PER_SAMPLE for b in BATCHES if b * p <= MAX_ELEMS or (b, p) == FORCED_G1]
    return out + [(b, p, 1) for p in ERR_OFFSET1 for b in (1, 3)]


def is_vec(per_sample, offset):
    return per_sample % 8 == 0 and offset == 0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def n_cu():
    n, lds = C.c_int(), C.c_int()
    L.check(L.lib.dpm_device_info(C.byref(n), C.byref(lds), C.create_string_buffer(64), 64))
    return n.value


class Handle:
    """a dpm_adaptive handle with its error word and time vectors in guarded arenas"""

    def __init__(self, sname="sd", order=2, tv_len=1, **kw):
        assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
        self.ns = make_schedule(sname)
        self.desc = desc_of(order, kw.pop("algo", ALGO_OF[sname]), kw.pop("solver", "dpmsolver"), **kw)
        self.h = C.c_void_p()
        L.check(L.lib.dpm_adaptive_create(self.ns._h, C.byref(self.desc), C.byref(self.h)))
        self.tv_len = tv_len
        self.e = G.Arena(torch.float32, 1, DEV, zero=True)
        self.tv = G.Arena(torch.float32, 6 * tv_len, DEV)
        self.begins = 0

    def __del__(self):
        if getattr(self, "h", None):
            torch.cuda.synchronize()
            L.lib.dpm_adaptive_destroy(self.h)
            self.h = None

    def reset(self):
        L.check(L.lib.dpm_adaptive_reset(self.h, _stream()))
        self.begins = 0

    def begin(self, case=None):
        p = case.ptrs() if case is not None else [None] * 4
        L.check(L.lib.dpm_adaptive_begin(self.h, p[0], p[1], p[2], p[3], case.n if case is not None else 0,
                                         G.CODE[case.dtype] if case is not None else L.DTYPE_F32, self.e.ptr, self.tv.ptr,
                                         self.tv_len, _stream()))
        self.begins += 1

    def live(self):
        """reset + the first begin without a state: e_dev is zero and the controller runs"""
        self.reset()
        self.begin()
        return self

    def set_e(self, value):
        self.e.payload_bits().copy_(torch.from_numpy(np.array([value], dtype=F32).view(np.int32)))

    def read_e(self):
        """*e_dev as fp32, after checking the floats on either side of it"""
        raw = self.e.raw.cpu()
        guards = torch.cat([raw[:self.e.lead], raw[self.e.lead + 1:]])
        assert bool((guards == G.FILL[4]).all()), "a float next to e_dev was overwritten"
        return raw[self.e.lead:self.e.lead + 1].numpy().view(F32)[0]

    def poll(self):
        torch.cuda.synchronize()
        v = [C.c_int(-1) for _ in range(4)]
        L.check(L.lib.dpm_adaptive_poll(self.h, *[C.byref(x) for x in v]))
        return dict(done=v[0].value, nfe=v[1].value, iterations=v[2].value, accepted=v[3].value)

    def done_at(self, j):
        return L.lib.dpm_adaptive_done_at(self.h, j)

    def error(self, ops, batch, per_sample, dtype):
        L.check(L.lib.dpm_adaptive_error(self.h, ops[0].ptr, ops[1].ptr, ops[2].ptr, batch, per_sample, G.CODE[dtype],
                                         self.e.ptr, _stream()))
        torch.cuda.synchronize()
        return self.read_e()


# ------------------------------------------------------------------------------------------------
# (a) error norm
# ------------------------------------------------------------------------------------------------
_POOL = {}


def pool(n):
    """three fp32 streams shared by every cell (generated once): x_lower, the step x_higher - x_lower, x_prev"""
    if "p" not in _POOL or _POOL["p"][0].numel() < n:
        g = torch.Generator().manual_seed(20240611)
        size = max(n, FORCED_G1[0] * FORCED_G1[1] + 4096)
        _POOL["p"] = [torch.randn(size, generator=g), 0.02 * torch.randn(size, generator=g), torch.randn(size, generator=g)]
    return _POOL["p"]


def error_operands(batch, per, dtype, offset=0, edit=None):
    """(arenas of x_lower, x_higher, x_prev on the GPU, the same values as fp32 [batch, per] arrays); `edit(l, h, p)` may
    change the fp32 tensors before they are rounded to `dtype`"""
    n, skip = batch * per, (per * 7 + batch * 13) % 4096
    a, d, c = (t[skip:skip + n].clone() for t in pool(n + 4096))
    l = a.to(dtype).float()
    h, p = l + d, c
    if edit is not None:
        edit(l.view(batch, per), h.view(batch, per), p.view(batch, per))
    ts = [t.to(dtype) for t in (l, h, p)]
    es = ts[0].element_size()
    arenas = [G.Arena(dtype, n, DEV, offset, bits=t.view(G._INT[es])) for t in ts]
    return arenas, [t.float().numpy().reshape(batch, per) for t in ts]


def check_error_cell(hd, batch, per, dtype, offset=0, edit=None, what=""):
    """one cell through both entry points; returns the double's (E_b, E_max)"""
    what = "%s %s batch=%d per_sample=%d offset=%d" % (what, G._name(dtype), batch, per, offset)
    ops, vals = error_operands(batch, per, dtype, offset, edit)
    want_b, want = AD.error_double(*vals, ATOL, RTOL)
    got = []
    for _ in range(2):                                     # the same launch twice: a fixed summation order, the same bits
        hd.set_e(0.0)
        got.append(hd.error(ops, batch, per, dtype))
    AD.check_error(got[0], want, "dpm_adaptive_error " + what)
    assert got[0].tobytes() == got[1].tobytes(), ("not deterministic", what, got)
    eo = G.Arena(torch.float32, batch + 1, DEV)
    outs = []
    for _ in range(2):
        L.check(L.lib.dpm_adaptive_error_launch(ops[0].ptr, ops[1].ptr, ops[2].ptr, ATOL, RTOL, eo.ptr, batch, per, G.CODE[dtype],
                                                _stream()))
        torch.cuda.synchronize()
        raw = eo.raw.cpu()
        assert bool((raw[:eo.lead] == G.FILL[4]).all()) and bool((raw[eo.lead + batch + 1:] == G.FILL[4]).all()), what
        outs.append(raw[eo.lead:eo.lead + batch + 1].numpy().view(F32).copy())
    AD.check_error(outs[0][:batch], want_b, "dpm_adaptive_error_launch " + what)
    AD.check_error(outs[0][batch], want, "dpm_adaptive_error_launch maximum " + what)
    assert outs[0].tobytes() == outs[1].tobytes(), ("not deterministic", what)
    for k, a in zip(("x_lower", "x_higher", "x_prev"), ops):
        a.verify("error norm %s %s" % (what, k))
    return want_b, want


@gpu
def test_error_cells_meet_the_coverage_rule():
    """on this device's compute-unit count the cells run G = 1, 2, 3, 64 and a value in between, the vector and the scalar route
    at G > 1, a chunk rounding that overshoots the sample, and a splittable sample in a batch that forces G = 1"""
    cu = n_cu()
    cells = error_cells()
    assert len({(b, p) for b, p, o in cells if o == 0}) >= 55 and {p for b, p, o in cells if o == 0} == set(PER_SAMPLE)
    assert {b for b, p, o in cells} == set(BATCHES) and len({p for b, p, o in cells if o == 1}) == 3
    assert all(b * p <= MAX_ELEMS or (b, p) == FORCED_G1 for b, p, o in cells)
    gs = {(b, p, o): AD.plan_G(b, p, cu) for b, p, o in cells}
    print("n_cu = %d; G values: %s" % (cu, sorted(set(gs.values()))))
    assert {1, 2, 3, 64} <= set(gs.values()) and any(3 < g < 64 for g in gs.values())
    assert any(g > 1 and is_vec(p, o) for (b, p, o), g in gs.items())
    assert any(g > 1 and o == 1 for (b, p, o), g in gs.items()) and any(g > 1 and p % 8 for (b, p, o), g in gs.items())
    assert any(g > 1 and AD.chunk(p, g) * g > p for (b, p, o), g in gs.items())
    assert any(g > 1 and p - (g - 1) * AD.chunk(p, g) < AD.chunk(p, g) for (b, p, o), g in gs.items())     # a ragged last chunk
    assert any(g == 1 and p >= 16384 and b > 1 for (b, p, o), g in gs.items())
    assert AD.plan_G(1, 524288, cu) == 64 and AD.plan_G(64, 524288, cu) < 64 and 1 < AD.plan_G(3, 65544, cu) < 64  # the regrow sequence


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=G._name)
def test_error_norm_sweep(dtype):
    hd = Handle().live()
    for batch, per, offset in error_cells():
        check_error_cell(hd, batch, per, dtype, offset)


def _value_cases(batch, per):
    """name -> edit of the fp32 [batch, per] tensors (l, h, p)"""
    def peak(b):
        def f(l, h, p):
            h[b] = l[b] + 0.5
        return f

    def zero(l, h, p):
        h.copy_(l)

    def crossover(l, h, p):                    # |x_lower|, |x_prev| below, at and above atol / rtol = 0.156
        c = ATOL / RTOL
        for i, (a, b) in enumerate([(0.5 * c, 0.25 * c), (c, 0.5 * c), (0.5 * c, c), (2 * c, 0.5 * c), (0.5 * c, 2 * c), (c, c)]):
            l[:, i::6] = a * torch.sign(l[:, i::6] + 1e-9)
            p[:, i::6] = b * torch.sign(p[:, i::6] + 1e-9)
            h[:, i::6] = l[:, i::6] + 0.01

    def overflow(l, h, p):                     # v = 1e19 / atol = 1.3e21, v * v is past fp32 (fp16 holds 1e19 as inf: inf again)
        l[0, 0], p[0, 0], h[0, 0] = 0.0, 0.0, 1e19

    def nan_last(l, h, p):
        h[-1, -1] = float("nan")

    def negzero(l, h, p):
        l[:, ::3], p[:, 1::3] = -0.0, -0.0
        h[:, ::3] = 0.004

    cases = {"max_first": peak(0), "max_middle": peak(batch // 2), "max_last": peak(batch - 1), "zero": zero,
             "crossover": crossover, "overflow": overflow, "nan_last_chunk": nan_last, "negative_zero": negzero}
    return cases


@gpu
@pytest.mark.parametrize("batch,per", [(5, 2049), (3, 24587)], ids=["G1", "G3"])
def test_error_norm_value_cases(batch, per):
    hd = Handle().live()
    assert AD.plan_G(batch, per, n_cu()) == (1 if per < 16384 else 3)
    for dtype in DTYPES:
        for name, edit in _value_cases(batch, per).items():
            e_b, e = check_error_cell(hd, batch, per, dtype, 0, edit, name)
            if name.startswith("max_"):
                b = {"max_first": 0, "max_middle": batch // 2, "max_last": batch - 1}[name]
                assert int(np.argmax(e_b)) == b and e == e_b[b]
            if name == "zero":
                assert e == 0.0
            if name == "overflow":
                assert np.isinf(e) and np.isinf(e_b[0]) and np.isfinite(e_b[1:]).all()
            if name == "nan_last_chunk":
                assert np.isnan(e) and np.isnan(e_b[-1]) and np.isfinite(e_b[0])


@gpu
def test_error_word_keeps_the_maximum():
    """*e_dev <- max(*e_dev, E): a second launch without a begin leaves it, a larger preset stays, a smaller one is raised"""
    hd = Handle().live()
    for batch, per in ((3, 2048), (2, 16392)):
        ops, vals = error_operands(batch, per, torch.float32)
        want = AD.error_double(*vals, ATOL, RTOL)[1]
        first = hd.error(ops, batch, per, torch.float32)
        AD.check_error(first, want, "first launch")
        assert hd.error(ops, batch, per, torch.float32).tobytes() == first.tobytes()
        hd.set_e(float(want) * 4)
        assert hd.error(ops, batch, per, torch.float32) == F32(float(want) * 4)
        hd.set_e(float(want) / 4)
        assert hd.error(ops, batch, per, torch.float32).tobytes() == first.tobytes()
        hd.set_e(0.0)


@gpu
def test_error_scratch_regrows_and_counters_return_to_zero():
    """(batch 1, G 64), (batch 64, G 1), (batch 3, G > 1) and the first again on ONE handle: the scratch grows with batch and with
    batch x G, and every launch leaves the per-sample counters at zero for the next"""
    hd = Handle().live()
    cu = n_cu()
    seq = [(1, 524288), (64, 8200), (3, 65544), (1, 524288), (64, 8200), (17, 65544)]
    assert [AD.plan_G(b, p, cu) for b, p in seq[:2]] == [64, 1] and AD.plan_G(3, 65544, cu) > 1
    for i, (batch, per) in enumerate(seq):
        check_error_cell(hd, batch, per, torch.float32 if i % 2 == 0 else torch.float16, 0, None, "step %d of the sequence" % i)


# ------------------------------------------------------------------------------------------------
# (b) commit
# ------------------------------------------------------------------------------------------------
COMMIT_SIZES = [1, 3, 4, 5, 7, 8, 9, 2044, 2048, 2052, 65540]


def commit_cells(dtype, cu):
    es = torch.empty(0, dtype=dtype).element_size()
    out = [(n, o) for n in COMMIT_SIZES for o in (0, 1)]
    past = (8 * cu * 256 + 1) * (16 // es)                 # one 16-byte vector past the grid cap of the vector route
    out += [(past, 0)]
    if dtype is torch.float32:
        out += [(8 * cu * 256 + 3, 1)]                     # three elements past the cap of the scalar route
    return out


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=G._name)
def test_commit_copies_on_accept_and_writes_nothing_otherwise(dtype):
    hd = Handle()
    script = [2.0, 0.5, 0.0, 0.5]                          # reject, accept, accept with h = the whole range, accept: done
    rows = AD.controller_double(hd.ns._h, hd.desc, script + [0.5])
    assert [r["accept"] for r in rows] == [0, 0, 1, 1, 1, 0] and [r["done"] for r in rows] == [0, 0, 0, 0, 1, 1]
    for n, offset in commit_cells(dtype, n_cu()):
        case = AD.CommitCase(dtype, n, offset, seed=n % 97).on(DEV)
        hd.reset()
        hd.begin(case)                                     # the first begin after a reset
        torch.cuda.synchronize()
        case.verify(False)
        hd.set_e(script[0])
        hd.begin(case)
        torch.cuda.synchronize()
        case.verify(False)                                 # a rejected step
        hd.set_e(script[1])
        hd.begin(case)
        torch.cuda.synchronize()
        case.verify(True)                                  # an accepted one
        for e in script[2:]:
            hd.set_e(e)
            hd.begin(case)
        assert hd.poll()["done"] == 1
        case.verify(True)
        fresh = AD.CommitCase(dtype, n, offset, seed=n % 97 + 1).on(DEV)
        hd.set_e(0.5)
        hd.begin(fresh)                                    # a begin after done
        torch.cuda.synchronize()
        fresh.verify(False)


# ------------------------------------------------------------------------------------------------
# (c) controller
# ------------------------------------------------------------------------------------------------
TV_LENS = [1, 3, 255, 256, 257, 600]
ABOVE_ONE = float(np.nextafter(F32(1.0), F32(2.0)))
SCRIPTS = {
    "half": dict(e=[0.5] * 400, until_done=True),
    "alternating": dict(e=[0.5, 3.7] * 12),
    "one_and_its_successor": dict(e=[1.0, ABOVE_ONE] * 12),
    "zero": dict(e=[0.0] * 6),
    "huge": dict(e=[1e30] * 12),
    "inf": dict(e=[0.5, float("inf")] + [float("inf")] * 8, stalls_after=2),
    "ring_wrap": dict(e=[0.5] * 40 + [0.0, 0.5, 0.5, 0.5, 0.5], theta=0.7),
    "nan": dict(e=[0.5, float("nan"), 0.5, 0.5]),
}
WORST = {"ulps": 0, "dt": 0.0}
# worst distance of a device t_eval from the double's, measured on an MI355X (256 CUs) over every script, schedule and order of
# this file: 0 ulps -- the device's interpolation, logf and expf gave the host planner's bits in every begin
T_EVAL_ULPS_MEASURED = 0
T_ERR = 1e-5


def _bits(v):
    return int(np.array(v, dtype=F32).view(np.int32))


def run_script(sname, order, name, tv_len):
    """drive one handle through a script, one begin at a time, and hold every begin against the double's row"""
    sc = SCRIPTS[name]
    hd = Handle(sname, order, tv_len, **({"theta": sc["theta"]} if "theta" in sc else {}))
    rows = AD.controller_double(hd.ns._h, hd.desc, sc["e"])
    if sc.get("until_done"):
        first = next(i for i, r in enumerate(rows) if r["done"])
        assert first + 3 < len(rows), "the script is too short to end"
        rows = rows[:first + 4]
    script = sc["e"][:len(rows) - 1]
    case = AD.CommitCase(torch.float32, 8, 0, seed=order).on(DEV)
    xa, fill = case.arenas["x"], torch.full((6 * tv_len,), G.FILL[4], dtype=torch.int32, device=DEV)
    hd.reset()
    prev_te0 = None
    for k, row in enumerate(rows):
        what = "%s order %d script %s begin %d" % (sname, order, name, k)
        mark = torch.full((8,), 0x3F000000 + k, dtype=torch.int32)
        xa.payload_bits().copy_(mark)
        hd.tv.payload_bits().copy_(fill)
        if k > 0:
            hd.set_e(script[k - 1])
        hd.begin(case)
        st = hd.poll()
        assert st == {q: row[q] for q in ("done", "nfe", "iterations", "accepted")}, (what, st, row)
        assert hd.done_at(k) == row["done"], what
        assert hd.read_e() == 0.0, what                                        # the begin clears the word it read
        x_now = xa.payload_bits().cpu()
        assert torch.equal(x_now, case.bits["x_higher"] if row["accept"] else mark), (what, "accept", row["accept"])
        raw = hd.tv.raw.cpu()
        lead, end = hd.tv.lead, hd.tv.lead + 6 * tv_len
        assert bool((raw[:lead] == G.FILL[4]).all()) and bool((raw[end:] == G.FILL[4]).all()), (what, "guard behind the time vectors")
        tv = raw[lead:end].reshape(6, tv_len)
        if not row["live"]:
            assert bool((tv == G.FILL[4]).all()), (what, "time vectors written after done")
            continue
        assert bool((tv == tv[:, :1]).all()), (what, "a time vector with two values")
        assert not bool((tv == G.FILL[4]).any()), (what, "a time vector entry not written")
        got = tv[:, 0].numpy().view(F32)
        for j in range(3):
            te, ti = got[2 * j], got[2 * j + 1]
            assert _bits(ti) == _bits(AD.t_input_of(hd.ns._h, te)), (what, j, te, ti)
            want = row["times"][j][0]
            d, dt = AD.ulps(te, want), abs(float(te) - float(want))
            WORST["ulps"], WORST["dt"] = max(WORST["ulps"], d), max(WORST["dt"], dt)
            assert dt <= T_ERR, (what, j, te, want)
            assert d <= 2 * T_EVAL_ULPS_MEASURED, (what, j, te, want, d)
        if k > 0 and not row["accept"]:
            assert _bits(got[0]) == prev_te0, (what, "t_eval[0] moved on a rejected step")
        if sc.get("stalls_after") and k > sc["stalls_after"]:
            assert _bits(got[0]) == prev_te0 and row["done"] == 0, (what, "progress with h = 0")
        prev_te0 = _bits(got[0])
    for k in range(max(0, len(rows) - 32), len(rows)):                         # the ring keeps the last 32 verdicts
        assert hd.done_at(k) == rows[k]["done"], (sname, order, name, k)
    case.arenas["x_lower"].verify("x_lower"), case.arenas["x_higher"].verify("x_higher")
    return hd, rows


CONTROLLER_RUNS = [(s, o) for s in ("sd", "vp_linear", "cosine1000") for o in (2, 3)]


def tv_len_of(run_index, script_index):
    return TV_LENS[(run_index + script_index) % len(TV_LENS)]


@gpu
@pytest.mark.parametrize("sname,order", CONTROLLER_RUNS)
def test_controller_against_the_double(sname, order):
    """every begin of every script: accept (through the commit), nfe, accepted, iterations, done, the ring -- all exact; the time
    vectors: 6 x tv_len floats, rows constant, t_input bit-equal to the formula on the device's own t_eval.  t_eval against the
    double is not promised bit for bit (the device evaluates logf, expf and the interpolation itself): |dt| <= t_err = 1e-5
    always (more is a bug, not a tolerance), and at most twice the worst distance measured on an MI355X.  Measured: 0 fp32 ulps
    over all scripts, schedules and orders (T_EVAL_ULPS_MEASURED), so the assertion is bit equality with the host planner."""
    i = CONTROLLER_RUNS.index((sname, order))
    names = [n for n in SCRIPTS if n != "nan"]
    assert {tv_len_of(r, s) for r in range(len(CONTROLLER_RUNS)) for s in range(len(names))} == set(TV_LENS)
    for j, name in enumerate(names):
        hd, rows = run_script(sname, order, name, tv_len_of(i, j))
        if name == "ring_wrap":
            assert len(rows) > 40 and rows[-1]["done"] == 1 and rows[40]["done"] == 0
        if name == "inf":
            assert rows[-1]["done"] == 0 and rows[-1]["h"] == 0
    print("t_eval against the double, %s order %d and before: worst %d ulps, %.3g" % (sname, order, WORST["ulps"], WORST["dt"]))


# ------------------------------------------------------------------------------------------------
# the NaN estimate
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sname,order", [("sd", 3), ("vp_linear", 2)])
def test_nan_estimate_ends_the_run_with_its_own_verdict(sname, order):
    """script 0.5, NaN: the begin that reads the NaN rejects, sets done = 2 (poll and done_at), writes no time vector -- they keep
    their last finite values -- and every later launch of the handle is a no-op"""
    hd, rows = run_script(sname, order, "nan", 3)
    assert [r["done"] for r in rows] == [0, 0, 2, 2, 2] and [r["accept"] for r in rows] == [0, 1, 0, 0, 0]
    assert hd.poll()["done"] == 2 and hd.done_at(2) == 2 and hd.done_at(1) == 0
    ops, _ = error_operands(2, 2048, torch.float32)
    assert hd.error(ops, 2, 2048, torch.float32) == 0.0                      # dpm_adaptive_error of a finished run


@gpu
@pytest.mark.parametrize("order", [2, 3])
def test_nan_network_raises_on_the_device_path(order):
    """a network that returns NaN on the default (device-side) path: FloatingPointError with the host loop's message instead of
    adaptive_max_iterations begins; the network is called for at most adaptive_lookahead + 2 iterations and never with a
    non-finite time"""
    ns = make_schedule("sd")
    calls, bad = [], []

    def net(xx, t):
        calls.append(1)
        if not bool(torch.isfinite(t).all()):
            bad.append(t)
        return xx * float("nan")
    dpm = D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++")
    assert dpm.adaptive_on_device
    dpm.adaptive_max_iterations = 64
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 3, 8, 8)).astype(F32)).to(DEV)
    with pytest.raises(FloatingPointError, match="error estimate is NaN at t = 1.0"):
        dpm.sample(x, method="adaptive", order=order, t_end=1e-3)
    assert not bad and 0 < len(calls) <= (int(dpm.adaptive_lookahead) + 2) * order, (len(calls), dpm.adaptive_lookahead)


# ------------------------------------------------------------------------------------------------
# (d) stage launches with device-resident coefficients
# ------------------------------------------------------------------------------------------------
STAGE_PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
               (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)]
STAGE_CONFIGS = [(2, "dpmsolver"), (3, "dpmsolver"), (3, "taylor")]
STAGE_VARIANTS = [("uncond", "noise"), ("classifier-free", "noise"), ("uncond", "v"), ("classifier-free", "v")]
STAGE_BOUND = 1e-5                                   # of max |want|: the project's bar for a trajectory against the reference


def host_records(hd, s, t):
    """the five stage records of the iteration s -> t from the host planner (dpm_coef_singlestep, dpm_coef_prologue)"""
    d, order = hd.desc, hd.desc.order

    def fill(o, r1, r2):
        st = (L.Stage * 3)()
        L.check(L.lib.dpm_coef_singlestep(hd.ns._h, d.algorithm_type, d.solver_type, o, float(s), float(t), r1, r2, 0, st))
        return [st[i].copy() for i in range(o)]
    if order == 2:
        lo, hi = fill(1, 0.0, 0.0), fill(2, 0.5, 0.0)
        recs = [lo[0], lo[0].copy(), hi[0], hi[1], hi[1].copy()]
    else:
        lo, hi = fill(2, 1.0 / 3.0, 0.0), fill(3, 1.0 / 3.0, 2.0 / 3.0)
        recs = [lo[0], lo[1], hi[0], hi[1], hi[2]]
    for r in recs:
        L.check(L.lib.dpm_coef_prologue(hd.ns._h, r.t_eval, d.model_type, d.guidance, d.guidance_scale, C.byref(r)))
    return recs


def stage_handle(order, solver, guidance, model):
    kw = dict(model_type=L.MODEL[model], guidance=L.GUIDE[guidance], guidance_scale=2.5 if guidance != "uncond" else 1.0)
    hd = Handle("sd", order, 1, solver=solver, **kw).live()
    row = AD.controller_double(hd.ns._h, hd.desc, [])[0]
    tmpl = []
    for i in range(5):
        st = L.Stage()
        L.check(L.lib.dpm_adaptive_stage_template(hd.h, i, C.byref(st)))
        tmpl.append(st)
    recs = host_records(hd, row["s"], row["t"])
    for a, b in zip(tmpl, recs):
        assert (a.form, a.flags, a.model_type, a.guidance, a.xe_src) == (b.form, b.flags, b.model_type, b.guidance, b.xe_src)
    return hd, tmpl, recs


def stage_launch(hd, which, tmpl, dev, noop=False):
    rc = L.lib.dpm_adaptive_stage_launch(hd.h, which, C.byref(tmpl), C.byref(dev.b), _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    dev.verify(noop=noop)
    return {k: dev.arenas[k].payload() for k in sorted(dev.written)}


def stage_cells():
    return [(n, 0) for n in SIZES] + [(n, 1) for n in OFFSET1]


@gpu
@pytest.mark.parametrize("p", range(len(STAGE_PAIRS)), ids=["%s-%s" % (G._name(s), G._name(e)) for s, e in STAGE_PAIRS])
def test_stage_launches_with_device_resident_coefficients(p):
    """every `which` of order 2 and of order 3 (dpmsolver and taylor: the SS3T form), unguided and classifier-free, noise and v
    networks, at the tile-edge sizes of test_gpu_edges.py: the structure checks of verify(); the vector route bit-equal to the
    same launch one element past the boundary (the one-element-per-lane kernel reading the same device coefficients); the
    values within 1e-5 of the tensor's scale of the numpy double on the host planner's records for the same (s, t)"""
    sd, ed = STAGE_PAIRS[p]
    cells = stage_cells()
    assert {o for n, o in cells} == {0, 1} and set(SIZES) <= {n for n, o in cells}
    k = 0
    for order, solver in STAGE_CONFIGS:
        for guidance, model in STAGE_VARIANTS:
            hd, tmpl, recs = stage_handle(order, solver, guidance, model)
            for which in range(5):
                # every (which, variant) at three sizes and one offset-1 size, both in rotation
                mine = [c for i, c in enumerate(cells) if (c[1] == 0 and (i + k) % 6 == 0) or c == (OFFSET1[k % 3], 1)]
                k += 1
                for n, offset in mine:
                    what = "order %d %s %s %s which %d n %d offset %d" % (order, solver, guidance, model, which, n, offset)
                    host = G.GuardedLaunch("adaptive", recs[which], n, sd, ed, offset=0, sep_xe=recs[which].xe_src == L.SRC_TMP,
                                           seed=n + which)
                    want = G.run_double(host)
                    got = stage_launch(hd, which, tmpl[which], host.on(DEV))
                    if offset == 1:
                        moved = G.GuardedLaunch("adaptive", recs[which], n, sd, ed, device=DEV, like=host, **dict(host.kw, offset=1))
                        scalar = stage_launch(hd, which, tmpl[which], moved)
                        for name in got:
                            assert torch.equal(got[name].view(G._INT[got[name].element_size()]),
                                               scalar[name].view(G._INT[got[name].element_size()])), (what, name)
                    for name, v in got.items():
                        w = want.arenas[name].payload().double()
                        err = float((v.double() - w).abs().max()) / float(w.abs().max())
                        assert err <= STAGE_BOUND, (what, name, err)
    assert k == len(STAGE_CONFIGS) * len(STAGE_VARIANTS) * 5


@gpu
def test_launches_of_a_finished_run_write_nothing():
    """after done, dpm_adaptive_stage_launch of every `which` and dpm_adaptive_error are no-ops"""
    for order, solver in STAGE_CONFIGS:
        hd, tmpl, recs = stage_handle(order, solver, "classifier-free", "noise")
        for e in (0.0, 0.5):
            hd.set_e(e)
            hd.begin()
        assert hd.poll()["done"] == 1
        for which in range(5):
            for n, offset, sd in ((2056, 0, torch.float32), (2055, 0, torch.float32), (2056, 1, torch.float32), (2056, 0, torch.float16)):
                dev = G.GuardedLaunch("adaptive", recs[which], n, sd, sd, device=DEV, offset=offset,
                                      sep_xe=recs[which].xe_src == L.SRC_TMP, seed=n)
                stage_launch(hd, which, tmpl[which], dev, noop=True)
        ops, _ = error_operands(3, 16392, torch.float32)
        assert hd.error(ops, 3, 16392, torch.float32) == 0.0
