"""The look-ahead of the device-side adaptive controller (dpm_solver_amd/adaptive.py, `adaptive_device`) without a GPU: the inputs
of the end-to-end runs of tests/test_gpu_run_ahead.py, shown here to wrap the controller's 32-entry status ring, and the number
of network calls such a run makes, derived from the host loop.

Inputs.  The sd schedule, x of [2,4,8,8], dpmsolver++, and a network whose coefficient is a square wave in the time label (exactly
rounded operations only: the same bits on the CPU and on the GPU, whatever the batch).  Every edge of the wave costs the
controller rejected steps.  With the tolerances of CASES the host loop on the numpy doubles of tests/kernel_double.py, replayed by
adaptive_double.controller_double, takes more than 40 begins -- past the 32 entries of the status ring -- and rejects steps, so
the verdicts are not one run of accepts; and no error estimate comes within 0.5 % of 1, the threshold of acceptance, so a
device whose estimates differ from the double's in the last place takes the same decisions.

Network calls.  Begin k is enqueued in front of iteration k; it decides iteration k - 1 and sets up iteration k.  Let U be the
useful iterations, NFE / order: begin U is the first whose verdict is `done`.  Before iteration `it` the host reads
done_at(it - 1 - look) once it > look, and breaks when it is set: the first such `it` is U + 1 + look.  The host has then
enqueued the iterations 0 .. U + look, each with `order` network calls:

    calls = order * (U + 1 + look),        look = adaptive_lookahead clamped to 0..24

-- look + 1 iterations after the last useful one, not `look`: with a look-ahead of 0 the host still enqueues iteration U before
it can read begin U's verdict.  `network_calls` is that count; `host_loop` restates the loop to check it.  The entry the host
reads, done_at(j), is entry j & 31 of the ring, and begin j + 32 overwrites it: the host is at most look + 1 <= 25 begins past j
when it reads, so it always reads begin j's own verdict."""
import numpy as np
import pytest
import torch

import adaptive_double as AD
import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import kernel_double as KD
from engine_cases import make_schedule
from test_adaptive_double_host import desc_of

F32 = np.float32
SHAPE = (2, 4, 8, 8)
T_END = 1e-3
# order -> the tolerances of its run
CASES = {2: dict(atol=2e-4, rtol=2e-3), 3: dict(atol=1e-3, rtol=1e-2)}
LOOKAHEADS = (0, 1, None, 24, 100, -3)             # None: the class default; 100 is clamped to 24, -3 to 0
RING = 32                                          # entries of the status ring (dpm_adaptive_done_at reads entry j & 31)


def net(x, t):
    """elementwise in the row and exactly rounded; the coefficient of the quadratic term jumps between 0.1 and 0.3 every 100
    of the sd schedule's 1000 time labels"""
    xf = x.float()
    xc = torch.clamp(xf, -2.0, 2.0)
    tf = t.float().reshape(-1, 1, 1, 1)
    wave = torch.remainder(torch.floor(tf / 100.0), 2.0)
    return (0.5 * xf + 0.1 * xc * xc * (1.0 + 2.0 * wave) + 0.0001 * tf).to(x.dtype)


def x_T():
    return 2.0 * torch.randn(SHAPE, generator=torch.Generator().manual_seed(230))


def clamped(lookahead):
    return min(max(int(D.DPM_Solver.adaptive_lookahead if lookahead is None else lookahead), 0), 24)


def network_calls(useful, lookahead, order):
    """network calls of a device-side adaptive run with `useful` = NFE / order useful iterations"""
    return order * (useful + 1 + clamped(lookahead))


def host_loop(done, look, max_it=100000):
    """the loop of adaptive_device on a device that has always run every begin the host waits for: `done[k]` the verdict after
    begin k (set for good from its first set entry on).  Returns (iterations enqueued, the ring entries it read as (j, begins
    enqueued when it read))"""
    at = lambda j: done[j] if j < len(done) else done[-1]
    it, read = 0, []
    while it < max_it:
        if it > look:
            j = it - 1 - look
            read.append((j, it))                    # begins 0 .. it - 1 are enqueued
            if at(j):
                break
        it += 1
    return it, read


def double_run(order, monkeypatch):
    """the host loop on the numpy doubles: (the E sequence it saw, controller_double's rows, the NFE it printed)"""
    KD.install_cpu_double(monkeypatch, S, D)
    ns = make_schedule("sd")
    dpm = D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++")
    dpm.adaptive_on_device = False
    seen, err = [], S._adaptive_error

    def record(*a):
        e = err(*a)
        seen.append(F32(e.item()))
        return e
    monkeypatch.setattr(S, "_adaptive_error", record)
    import contextlib
    import io
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        dpm.sample(x_T(), method="adaptive", order=order, t_end=T_END, **CASES[order])
    nfe = int(out.getvalue().strip().rsplit(" ", 1)[1])
    d = desc_of(order, "dpmsolver++", t_end=T_END, **CASES[order])
    return seen, AD.controller_double(ns._h, d, seen), nfe


@pytest.mark.parametrize("order", [2, 3])
def test_the_inputs_wrap_the_status_ring_and_reject_steps(monkeypatch, order):
    seen, rows, nfe = double_run(order, monkeypatch)
    begins = len(rows)
    assert begins == len(seen) + 1 and rows[-1]["done"] == 1 and [r["done"] for r in rows[:-1]] == [0] * (begins - 1)
    assert rows[-1]["nfe"] == nfe == order * len(seen)
    assert begins >= 40 > RING, begins                                          # past the 32-entry ring
    rejected = sum(1 for r in rows[1:] if not r["accept"])
    assert rejected >= 1 and rows[-1]["accepted"] == len(seen) - rejected, (rejected, len(seen))
    assert any(not r["accept"] for r in rows[RING + 1:]), "no rejected step behind the ring's first wrap"
    # no estimate near the threshold: the decisions do not hang on the last place of E
    assert min(abs(float(e) - 1.0) for e in seen) > 5e-3
    print("order %d: %d begins, %d rejected, NFE %d" % (order, begins, rejected, nfe))


def test_network_calls_is_the_host_loop_restated():
    """calls = order * (U + 1 + look) for every clamped look-ahead, on verdict rows of any length; the host never reads a ring
    entry that a later begin could have overwritten"""
    for useful in (1, 2, 7, 31, 32, 33, 57, 200):
        done = [0] * useful + [1]
        for look in range(0, 25):
            its, read = host_loop(done, look)
            assert its == useful + 1 + look, (useful, look, its)
            for order in (2, 3):
                assert network_calls(useful, look, order) == order * its
            # entry j & 31 still holds begin j's verdict: fewer than 32 further begins were enqueued when it was read
            assert all(0 < begins - j <= 25 < RING for j, begins in read), (useful, look)
    assert [clamped(v) for v in LOOKAHEADS] == [0, 1, 1, 24, 24, 0] and clamped(24.9) == 24
    # the docstring of adaptive_device states this count
    assert "lookahead + 1" in S.DPM_Solver._adaptive_device.__doc__
