#!/usr/bin/env python3
"""Continuous batching without lockstep: what a stage tick costs when 32 requests sit at different positions of their
trajectories.

Workload (bench.py's, with lockstep removed): 32 requests of [256,4,64,64] fp16, DPM-Solver++(2M), 20 steps, frozen eps
(every request's network output is a fixed tensor: the ticks measure the stage launches alone), steady state.  Request r
sits at stage (k + off_r) mod 20 at tick k, off_r = 20 r / 32, so every tick mixes first-order, second-order and final
stages; a request that finishes starts over from its x_T.  Three ways to advance one tick:

    a  lockstep   the same requests all at stage k mod 20: ONE dpm_stage_launch_multi (stage_kernel_multi, 32 per launch)
    b  staggered  the staggered positions, dpm_stage_launch_multi with per-request stage records (stage_kernel_het)
    c  today      the staggered positions with dpm_launch_opts.no_fuse: one dpm_stage_launch per request (stage_kernel)

Per mode: HIP events around `--ticks` back-to-back ticks after `--warmup` ticks -> us per request-stage and the fraction of
8 TB/s (5 n s bytes per second-order request-stage, 4 n s for the first and the last stage of a trajectory).  Kernel times
come from a separate run under rocprofv3 (the three modes launch kernels of three different names):

    python tools/staggered_requests.py --out DIR/events.json
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/staggered_requests.py --ticks 100 --repeat 1
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dpm_solver_amd as D  # noqa: E402
from dpm_solver_amd import _lib as L  # noqa: E402
from dpm_solver_amd.launch_list import _FastRun  # noqa: E402

R, STEPS, SHAPE = 32, 20, (256, 4, 64, 64)
PEAK = 8.0e12  # bytes / s


def build(dev):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: x, ns), ns, algorithm_type="dpmsolver++", state_dtype=torch.float16)
    plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N)
    assert len(plan.stages) == STEPS
    g = torch.Generator(device=dev).manual_seed(0)
    keep, recs = [plan], []      # recs[r][i] = (Stage, Buffers) of request r at stage i
    for _ in range(R):
        fr = _FastRun(dpm, plan, SHAPE, torch.float16, dev, False)
        x_T = torch.randn(SHAPE, generator=g, device=dev).half()
        eps = (0.5 * torch.randn(SHAPE, generator=g, device=dev)).half()
        out = torch.empty(SHAPE, dtype=torch.float16, device=dev)
        keep += [fr, x_T, eps, out]
        row = []
        for i, b0 in enumerate(fr.bufs):
            b = L.Buffers()
            C.memmove(C.byref(b), C.byref(b0), C.sizeof(L.Buffers))
            xi, xei, _ = plan.roles[i]
            if xi == 0:
                b.x = x_T.data_ptr()
            if xei == 0 and xi != 0:
                b.xe = x_T.data_ptr()
            if i == fr.last:
                b.x_out = out.data_ptr()
            b.e0, b.eps_dtype = eps.data_ptr(), L.DTYPE_F16
            row.append((fr.stages[i], b))
        recs.append(row)
    return keep, recs


def stage_bytes(st, nbytes):
    """bytes one request-stage moves: x and eps (+ the cached model value of a second-order stage) in, x (+ m) out"""
    streams = 2 + (st.form == L.FORM_TWO) + 1 + bool(st.flags & L.F_STORE_M)
    return streams * nbytes


def ticks_of(mode, recs):
    """the STEPS distinct ticks of a mode: (stage records, buffer records, bytes moved), and the options they point at"""
    nbytes = int(np.prod(SHAPE)) * 2
    out = []
    opts = L.LaunchOpts()
    opts.per_request_stages = 1
    opts.no_fuse = 1 if mode == "c" else 0
    for k in range(STEPS):
        pos = [k % STEPS if mode == "a" else (k + (STEPS * r) // R) % STEPS for r in range(R)]
        sts = (L.Stage * R)(*[recs[r][pos[r]][0] for r in range(R)])
        bufs = (L.Buffers * R)(*[recs[r][pos[r]][1] for r in range(R)])
        if mode != "a":
            bufs[0].opts = C.pointer(opts)
        out.append((sts, bufs, sum(stage_bytes(recs[r][pos[r]][0], nbytes) for r in range(R))))
    return out, opts


def run(mode, recs, warmup, ticks, stream):
    tk, opts = ticks_of(mode, recs)

    def tick(k):
        sts, bufs, _ = tk[k % STEPS]
        L.check(L.lib.dpm_stage_launch_multi(sts, bufs, R, stream))
    for k in range(warmup):
        tick(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(warmup, warmup + ticks):
        tick(k)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) / 1e3
    moved = sum(tk[k % STEPS][2] for k in range(warmup, warmup + ticks))
    del opts
    return dict(mode=mode, ticks=ticks, us_per_request_stage=sec * 1e6 / (ticks * R), us_per_tick=sec * 1e6 / ticks,
                hbm_fraction=moved / sec / PEAK)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ticks", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3, help="rounds of a, b, c (alternating)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("staggered_requests.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, recs = build(dev)
    rows = [run(m, recs, a.warmup, a.ticks, stream) for _ in range(a.repeat) for m in "abc"]
    res = {"workload": "32 x [256,4,64,64] fp16, DPM-Solver++(2M), 20 steps, frozen eps, staggered positions", "rows": rows}
    for m in "abc":
        v = [r["us_per_request_stage"] for r in rows if r["mode"] == m]
        f = [r["hbm_fraction"] for r in rows if r["mode"] == m]
        res[m] = dict(us_per_request_stage_median=float(np.median(v)), hbm_fraction_median=float(np.median(f)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    del keep


if __name__ == "__main__":
    main()
