#!/usr/bin/env python3
"""Requests of different shapes in flight: what a stage tick of 16 requests of 16 shapes costs in one launch and in sixteen.

Workload: 16 DPM-Solver++(2M) requests `[b,4,64,64]`, b = 16, 32, ..., 256 -- all shapes different, 35.7 M elements and, in
fp16, 356 MB of streams per tick, more than the Infinity Cache: every input comes from HBM.  20 steps, request r at stage
(k + 20 r / 16) mod 20 of tick k, frozen network output (the ticks measure the stage launches alone).  Modes, all through
dpm_stage_launch_multi with per-request stage records:

    m  mixed, fuse_shapes = 1    one stage_kernel_shapes launch per tick
    p  mixed, fuse_shapes = 0    the parent commit's behaviour for this call: no two requests agree on n, 16 lone launches
    u  uniform, fuse_shapes = 0  16 requests of [136,4,64,64] -- the same elements per tick in one shape: stage_kernel_het
    U  uniform, fuse_shapes = 1  the same call with the flag set: a group of one n takes the kernels it always took

The script drives the C entry point only, so modes p and u also run in a checkout of an older commit (where the options have
no fuse_shapes, modes m and U are refused).  HIP events around `--ticks` back-to-back ticks after `--warmup`, `--repeat` rounds
over the modes, alternating; --ticks defaults to a region of a second or more per mode.

    python tools/pool_shapes.py --dtype fp16 --out DIR/events.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/pool_shapes.py --ticks 100 --repeat 1
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

R, STEPS = 16, 20
BATCHES = {"mixed": [16 * (r + 1) for r in range(R)], "uniform": [136] * R}
DTYPES = {"fp16": (torch.float16, L.DTYPE_F16), "fp32": (torch.float32, L.DTYPE_F32)}
MODES = {"m": ("mixed", 1), "p": ("mixed", 0), "u": ("uniform", 0), "U": ("uniform", 1)}
HAS_FLAG = hasattr(L.LaunchOpts, "fuse_shapes")


def build(dev, dtype, which):
    """recs[r][i] = (Stage, Buffers) of request r at stage i, for the batch sizes BATCHES[which]"""
    td, code = DTYPES[dtype]
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: x, ns), ns, algorithm_type="dpmsolver++", state_dtype=td)
    plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N)
    g = torch.Generator(device=dev).manual_seed(0)
    keep, recs = [plan], []
    for r in range(R):
        shape = (BATCHES[which][r], 4, 64, 64)
        fr = _FastRun(dpm, plan, shape, td, dev, False)
        x_T = torch.randn(shape, generator=g, device=dev).to(td)
        eps = (0.5 * torch.randn(shape, generator=g, device=dev)).to(td)
        out = torch.empty(shape, dtype=td, device=dev)
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
            b.e0, b.eps_dtype = eps.data_ptr(), code
            row.append((fr.stages[i], b))
        recs.append(row)
    return keep, recs


def ticks_of(recs, fuse_shapes):
    """the STEPS distinct ticks: (stage records, buffer records); request 0's options carry the flags"""
    out, keep = [], []
    for k in range(STEPS):
        pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
        sts = (L.Stage * R)(*[recs[r][pos[r]][0] for r in range(R)])
        bufs = (L.Buffers * R)(*[recs[r][pos[r]][1] for r in range(R)])
        o = L.LaunchOpts()
        o.per_request_stages = 1
        if fuse_shapes:
            if not HAS_FLAG:
                sys.exit("pool_shapes.py: this library's dpm_launch_opts has no fuse_shapes (modes m and U need version 207)")
            o.fuse_shapes = 1
        bufs[0].opts = C.pointer(o)
        keep.append(o)
        out.append((sts, bufs))
    return out, keep


def run(recs, fuse_shapes, warmup, ticks, stream):
    tk, keep = ticks_of(recs, fuse_shapes)

    def tick(k):
        sts, bufs = tk[k % STEPS]
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
    del keep
    return dict(ticks=ticks, region_s=sec, us_per_tick=sec * 1e6 / ticks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp16")
    ap.add_argument("--modes", default="mpuU" if HAS_FLAG else "pu")
    ap.add_argument("--ticks", type=int, default=0, help="a multiple of 20; 0 = a second or more per mode (24000 fp16, 12000 fp32)")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3, help="rounds over the modes (alternating)")
    ap.add_argument("--label", default="", help="copied into the result (which library / commit this is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_shapes.py measures on the GPU; no device found")
    ticks = a.ticks or (24000 if a.dtype == "fp16" else 12000)
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    built = {w: build(dev, a.dtype, w) for w in sorted({MODES[m][0] for m in a.modes})}
    rows = []
    for _ in range(a.repeat):
        for m in a.modes:
            which, flag = MODES[m]
            rows.append(dict(mode=m, **run(built[which][1], flag, a.warmup, ticks, stream)))
    elems = {w: sum(BATCHES[w]) * 4 * 64 * 64 for w in BATCHES}
    res = {"workload": "16 x [b,4,64,64] %s, 2M, 20 steps, staggered, frozen eps; mixed b = 16..256, uniform b = 136" % a.dtype,
           "label": a.label, "device": torch.cuda.get_device_name(0), "library": os.path.relpath(L.LIB_PATH, ROOT),
           "version": int(L.lib.dpm_version()), "ticks": ticks, "warmup": a.warmup, "repeat": a.repeat,
           "elements_per_tick": elems, "rows": rows}
    for m in a.modes:
        v = [r["us_per_tick"] for r in rows if r["mode"] == m]
        res[m] = dict(us_per_tick_median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")
    del built


if __name__ == "__main__":
    main()
