"""The two mechanisms that keep the host correct when it is AHEAD of the device, on the MI355X with the device made slow.

Every other GPU test runs networks of a few elementwise operations: a host tick costs more than its GPU work, every event has
passed by the time it is looked at, and neither the slab pool's staging ring (slab.py: _RING pinned slots, each refilled behind
`_event_wait` on the event of its table copy) nor the adaptive controller's look-ahead (adaptive.py: the host enqueues up to 25
iterations past the last verdict it has read from a 32-entry ring) ever has to hold anything back.  Here the network carries
ordinary, bounded GPU work in front of it -- a chain of K matmuls on a scratch tensor, result discarded -- so that one network
call outlasts four host ticks.  K is sized in this module: h = the host time of one steady tick (a warm-up run of the same pool
with a synchronise per tick), the delay = the GPU time of one delayed network call (events), K = the smallest whose delay is at
least max(4 h, 1 ms) -- four host ticks must fit inside one network call for the first reuse of slot 0 to block.

Slab pools (the mixed pool of mixed_pool_cases, an apg=True pool, a pair=True pool; classifier-free, per-request conditions):
submit and step with no synchronisation until the pool drains, every result held; each must be the bits of the request alone
with no delay; a tick is one network call and one copy (two when it admits).  CONDITION: on every ring slot at least one wait
found its event not yet passed.  A device that never fell behind FAILS the test -- it would have shown nothing.

Adaptive: the inputs tests/test_adaptive_lookahead_host.py shows to wrap the status ring, adaptive_lookahead = 0, 1, the
default, 24, 100 and -3, each with the plain and with the delayed network: one result, one NFE (the CPU double's), and exactly
order * (U + 1 + look) network calls; with the delay and a look-ahead of 24 the device is caught iterations behind at the run's
final synchronise.  Only correct code runs here; what a broken ordering does is shown on the CPU (test_slab_staging_host.py).
Run on an MI355X:  pytest -m gpu
"""
import time

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import mixed_pool_cases as M
import test_adaptive_lookahead_host as AL
import test_gpu_slab_apg as APG
import test_gpu_slab_pair as PAIR
from dpm_solver_amd import _device as DV
from dpm_solver_amd.slab import _RING
from engine_cases import make_schedule
from test_gpu_slab_pool import _net
from test_slab_pair_host import OWN, REQS, SLOTS

gpu = pytest.mark.gpu
DEV = "cuda:0"
NET_CALLS = []
MAT = 2048                                        # the scratch matmuls: [MAT, MAT] fp32, long against their launch
SIZED = {}                                        # pool -> dict(h, delay, k), for the adaptive test and the printed record


class Delay:
    """K chained matmuls on a scratch tensor (an averaging matrix: every product stays finite), result discarded"""
    k = 0
    a = y = None

    @classmethod
    def work(cls):
        if cls.k:
            if cls.a is None:
                cls.a = torch.full((MAT, MAT), 1.0 / MAT, device=DEV)
                cls.y = torch.rand(MAT, MAT, device=DEV)
            y = cls.y
            for _ in range(cls.k):
                y = torch.mm(cls.a, y)


def _delayed(x, t, c=None):
    Delay.work()
    NET_CALLS.append(int(x.shape[0]))
    return _net(x, t, c)


@pytest.fixture(autouse=True)
def _no_delay_left_behind():
    yield
    Delay.k = 0


def _gpu_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def size_delay(name, h, call):
    """the smallest K whose delayed network call `call()` takes at least max(4 h, 1 ms) of GPU time (h in seconds)"""
    target = max(4.0 * h, 1e-3) * 1e3
    seen = {}

    def ms(k):                                     # the median of three, measured once per K
        if k not in seen:
            Delay.k = k
            seen[k] = sorted(_gpu_ms(call) for _ in range(3))[1]
        return seen[k]
    Delay.k = 4
    call()                                         # (the first matmul brings its library up)
    hi = 1
    while ms(hi) < target:
        hi *= 2
        assert hi <= 1 << 14, "no chain of matmuls reaches %.3f ms" % target
    lo = hi // 2                                   # ms(lo) < target <= ms(hi), or hi == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ms(mid) >= target else (mid, hi)
    delay = ms(hi)
    Delay.k = 0
    SIZED[name] = dict(h=h, delay=delay * 1e-3, k=hi)
    print("%s pool: h = %.3f ms per steady host tick, delay = %.3f ms per network call, K = %d matmuls of %d^2"
          % (name, h * 1e3, delay, hi, MAT))
    return hi


class Spy:
    """wraps dpm_solver_amd._device._event_wait and _copy_to_device (the real ones run): waits per ring slot, and those that
    found their event not yet passed"""

    def __init__(self, monkeypatch, pool):
        self.waits, self.blocked, self.copies = [0] * _RING, [0] * _RING, 0
        wait, copy = DV._event_wait, DV._copy_to_device

        def spy_wait(ev):
            if ev is not None:
                slot = next(k for k, g in enumerate(pool._ring) if g.ev is ev)
                self.waits[slot] += 1
                self.blocked[slot] += not ev.query()
            return wait(ev)

        def spy_copy(dst, src):
            self.copies += 1
            return copy(dst, src)
        monkeypatch.setattr(DV, "_event_wait", spy_wait)
        monkeypatch.setattr(DV, "_copy_to_device", spy_copy)


def drive(pool, ticks_of, submit, net_rows, timed=None):
    """submit request j on tick ticks_of[j] and step until the pool drains, with no synchronisation (timed: a list that takes
    the host seconds of every steady tick, each between two synchronises).  Per tick: ONE network call on the whole slab, one
    copy, two when the tick admits.  Returns {j: result}"""
    handles, got, tick = {}, {}, 0
    while tick <= max(ticks_of) or pool:
        for j, t in enumerate(ticks_of):
            if t == tick:
                handles[submit(pool, j)] = j
        nets, copies, waiting = len(NET_CALLS), pool.copies, len(pool._wait)
        if timed is not None:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = pool.step()
        dt = time.perf_counter() - t0
        admitted, copies = waiting - len(pool._wait), pool.copies - copies
        assert NET_CALLS[nets:] == [net_rows], "a tick is ONE network call on the whole slab"
        assert copies == 1 or (admitted and copies == 2), (tick, admitted, copies)
        if timed is not None and not admitted:
            timed.append(dt)
        for h, out in done.items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(ticks_of)))
    return got


def run_ahead(name, monkeypatch, make_pool, ticks_of, submit, net_rows, alone, net_call):
    """the three runs of one pool: warm-up with a synchronise per tick (h), the delayed run under the spy, every request alone"""
    timed = []
    drive(make_pool(), ticks_of, submit, net_rows, timed)
    h = float(np.median(timed))
    k = size_delay(name, h, net_call)
    pool = make_pool()
    spy = Spy(monkeypatch, pool)
    Delay.k = k
    got = drive(pool, ticks_of, submit, net_rows)          # no synchronisation until here; `got` holds every result
    Delay.k = 0
    torch.cuda.synchronize()
    print("%s pool: %d ticks, waits per ring slot %s, of which blocked %s" % (name, pool._tick, spy.waits, spy.blocked))
    SIZED[name].update(ticks=pool._tick, waits=list(spy.waits), blocked=list(spy.blocked))
    assert pool._tick >= 3 * _RING and spy.copies == pool.copies
    assert sum(spy.waits) == pool._tick - _RING                                  # one wait per tick once the ring has wrapped
    assert all(spy.blocked), \
        ("the device never fell behind the host on ring slot(s) %s: no wait there found its event pending, the ring was not "
         "exercised (h = %.3f ms, delay = %.3f ms, K = %d, blocked waits per slot %s)"
         % ([s for s in range(_RING) if not spy.blocked[s]], h * 1e3, SIZED[name]["delay"] * 1e3, k, spy.blocked))
    for j in sorted(got):
        want = alone(j)
        assert got[j].shape == want.shape and got[j].dtype == want.dtype, j
        assert torch.equal(got[j], want), (name, j)


# ----------------------------------------------------------------------------------------------------------------------------
# slab pools
# ----------------------------------------------------------------------------------------------------------------------------
_BETAS = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
NS = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - _BETAS).astype(np.float32)))


def _mixed_solver(dtype, cond=None, uncond=None, cxt=None):
    fn = D.model_wrapper(_delayed, NS, guidance_type="classifier-free", guidance_scale=3.0,
                         condition=torch.ones(1, 1, device=DEV) if cond is None else cond,
                         unconditional_condition=torch.zeros(1, 1, device=DEV) if uncond is None else uncond)
    return D.DPM_Solver(fn, NS, algorithm_type="dpmsolver++", correcting_xt_fn=cxt, state_dtype=dtype)


def _slab_call(rows, shape, dtype):
    """one network call of a pool's tick, for the event timing: the whole slab, a time and a condition per row"""
    x = torch.randn((rows,) + shape, device=DEV).to(dtype)
    t, c = torch.full((rows,), 500.0, device=DEV), torch.rand(rows, 1, device=DEV)
    return lambda: _delayed(x, t, c)


@gpu
def test_mixed_pool_with_the_device_behind(monkeypatch):
    """fp16, [4,16,16], 12 slots, the first 20 requests of mixed_pool_cases.ORDER: plain, UniPC, SDE and inpainting requests"""
    dtype = torch.float16
    sps = M.specs(M.ORDER[:20])
    assert {sp["kind"] for sp in sps} == set(M.KINDS)
    xs, conds, mbs = M.tensors(sps, dtype, DEV, NS, D.MaskBlend)
    run_ahead("mixed", monkeypatch, lambda: _mixed_solver(dtype).request_pool(slots=M.SLOTS, sde=True, inpaint=True),
              [sp["tick"] for sp in sps], lambda pool, j: M.submit(pool, sps[j], xs[j], conds[j], mbs[j], True), 2 * M.SLOTS,
              lambda j: M.alone(lambda c, u, cxt: _mixed_solver(dtype, c, u, cxt), sps[j], xs[j], conds[j], mbs[j], True),
              _slab_call(2 * M.SLOTS, M.SHAPE, dtype))


@gpu
def test_apg_pool_with_the_device_behind(monkeypatch):
    """records behind the rows and the running averages: the 24 staggered requests of test_gpu_slab_apg.py, 40 rows' worth, in 12
    slots -- requests wait, rows are reused under a momentum, and admissions go on for most of the run's 30 ticks"""
    dtype, shape = torch.float16, (4, 8, 8)
    monkeypatch.setattr(APG, "_counted", _delayed)
    reqs, xs, conds = APG._requests(24, shape)
    xs = [x.to(DEV).to(dtype) for x in xs]
    conds = [(c.to(DEV), u.to(DEV)) for c, u in conds]
    wrapper = (0.5, 10.0, -0.25)

    def submit(pool, j):
        _, kw, b, s, par = reqs[j]
        return pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], guidance_scale=s, apg=par, **kw)

    def alone(j):
        _, kw, b, s, par = reqs[j]
        return APG._solver(dtype, s, par, *[c.expand(b, -1) for c in conds[j]]).sample(xs[j], **kw)
    assert any(r[4][2] != 0 for r in reqs) and sum(r[2] for r in reqs) > 3 * 12
    run_ahead("apg", monkeypatch, lambda: APG._solver(dtype, 3.0, wrapper).request_pool(slots=12, apg=True),
              [r[0] for r in reqs], submit, 24, alone, _slab_call(24, shape, dtype))


@gpu
def test_pair_pool_with_the_device_behind(monkeypatch):
    """[3S, ...] slabs and a third copy: 8 slots, the 12 staggered requests of test_slab_pair_host.py"""
    dtype, shape = torch.float16, (4, 8, 8)
    monkeypatch.setattr(PAIR, "_counted", _delayed)
    g = torch.Generator().manual_seed(219)
    xs = [(2.0 * torch.randn((b,) + shape, generator=g)).to(DEV).to(dtype) for _, _, b in REQS]
    conds = [tuple(c.to(DEV) for c in (torch.rand(b if j % 2 else 1, 1, generator=g),
                                       torch.rand(1 if j % 3 else b, 1, generator=g) - 1.0,
                                       torch.rand(b if j % 4 == 2 else 1, 1, generator=g) + 0.5))
             for j, (_, _, b) in enumerate(REQS)]

    def submit(pool, j):
        s, scale2, nested = OWN[j]
        return pool.submit(xs[j], condition=conds[j][0], unconditional_condition=conds[j][1], condition2=conds[j][2],
                           guidance_scale=s, pair=(scale2, nested), **REQS[j][1])

    def alone(j):
        return PAIR._solver(dtype, *OWN[j], *[c.expand(REQS[j][2], -1) for c in conds[j]]).sample(xs[j], **REQS[j][1])
    run_ahead("pair", monkeypatch, lambda: PAIR._solver(dtype).request_pool(slots=SLOTS, pair=True),
              [r[0] for r in REQS], submit, 3 * SLOTS, alone, _slab_call(3 * SLOTS, shape, dtype))


# ----------------------------------------------------------------------------------------------------------------------------
# adaptive look-ahead
# ----------------------------------------------------------------------------------------------------------------------------
def _adaptive_k():
    """the delayed network of the slab pools: the mixed pool's K (sized here when that test has not run in this process)"""
    if "mixed" not in SIZED:
        dtype = torch.float16
        sps = M.specs(M.ORDER[:20])
        xs, conds, mbs = M.tensors(sps, dtype, DEV, NS, D.MaskBlend)
        timed = []
        drive(_mixed_solver(dtype).request_pool(slots=M.SLOTS, sde=True, inpaint=True), [sp["tick"] for sp in sps],
              lambda pool, j: M.submit(pool, sps[j], xs[j], conds[j], mbs[j], True), 2 * M.SLOTS, timed)
        size_delay("mixed", float(np.median(timed)), _slab_call(2 * M.SLOTS, M.SHAPE, dtype))
    return SIZED["mixed"]["k"]


@gpu
@pytest.mark.parametrize("order", [2, 3])
def test_adaptive_result_nfe_and_network_calls_at_every_lookahead(order, monkeypatch, capsys):
    with pytest.MonkeyPatch.context() as mp:                # the CPU double's run: how many useful iterations there are
        _, rows, nfe = AL.double_run(order, mp)
    useful = nfe // order
    assert len(rows) == useful + 1 >= 40
    k = _adaptive_k()
    ns = make_schedule("sd")
    calls, events, state = [], [], dict(armed=False, behind=None)

    def net(x, t):
        Delay.work()
        calls.append(1)
        out = AL.net(x, t)
        if state["armed"]:
            ev = torch.cuda.Event()
            ev.record()
            events.append(ev)
        return out
    sync = torch.cuda.Stream.synchronize

    def final_synchronise(stream):
        # adaptive_device's one wait: the last enqueue is behind it.  ONE query, of the network call twelve iterations back
        if state["armed"]:
            state["armed"], state["behind"] = False, not events[-12 * order].query()
        return sync(stream)
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", final_synchronise)
    dpm = D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++")
    assert dpm.adaptive_on_device and dpm.adaptive_lookahead == 1
    x = AL.x_T().to(DEV)
    assert dpm._adaptive_runs_on_device(x)
    sized = capsys.readouterr().out
    with capsys.disabled():
        print(sized, end="")
    results = []
    for delayed in (False, True):
        for look in AL.LOOKAHEADS:
            if look is None:
                dpm.__dict__.pop("adaptive_lookahead", None)  # the class default
            else:
                dpm.adaptive_lookahead = look
            Delay.k = k if delayed else 0
            state["armed"] = delayed and look == 24
            del calls[:], events[:]
            out = dpm.sample(x, method="adaptive", order=order, t_end=AL.T_END, **AL.CASES[order])
            Delay.k = 0
            what = (order, look, "delayed" if delayed else "plain")
            assert capsys.readouterr().out.strip() == "adaptive solver nfe %d" % nfe, what       # the CPU double's NFE
            assert len(calls) == AL.network_calls(useful, look, order), (what, len(calls), useful)
            results.append((what, out))
            if delayed and look == 24:
                assert state["behind"] is not None, "the final synchronise was not seen"
                assert state["behind"], \
                    ("the device was not behind the host at the run's final synchronise: the network call twelve iterations "
                     "back had already finished, the look-ahead of 24 was not exercised (%r)" % (SIZED["mixed"],))
    assert len(results) == 12
    for what, out in results[1:]:
        assert torch.equal(out, results[0][1]), (what, "differs from", results[0][0])
