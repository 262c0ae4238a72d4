#!/usr/bin/env python3
"""UniPC requests in flight: what a stage tick of 32 UniPC-2 requests costs when they sit at different positions of their plans.

Workload (tools/sde_requests.py's, with the UniPC plan): 32 requests of [256,4,64,64], UniPC-2 (bh2), 20 steps, frozen network
output (the ticks measure the stage launches alone; 32 x 5-6 streams exceed the Infinity Cache, so every input comes from HBM).
Modes, all through dpm_stage_launch_multi:

    a  lockstep   all requests at stage k mod 20                         (stage_kernel_multi, one launch per tick)
    b  staggered  request r at stage (k + 20 r / 32) mod 20              (stage_kernel_het_unipc, 16 requests per launch): every
                  tick holds stage-0 (first-order), stage-1 (first-order corrector), steady and tail requests
    c  no_fuse    the staggered positions, one launch per request        (stage_kernel)
    L  tools/unipc_stage.py's figure in the same process: the steady UniPC-2 stage in lockstep (dpm_plan_run_multi, the
       library's own event-bracketed launches)

Over 20 ticks modes a, b and c advance every request through every stage once: the same request-stages, grouped differently.
The script drives the C entry point only, so it also runs in a checkout of an older commit: where the per-request-stage launch
has no UniPC kernel, mode b measures UniPC stages request by request.  HIP events around `--ticks` back-to-back ticks after
`--warmup`; kernel names and times come from a separate run under rocprofv3:

    python tools/unipc_pool.py --dtype fp16 --out DIR/events.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/unipc_pool.py --ticks 100 --repeat 1 --modes abc
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dpm_solver_amd as D  # noqa: E402
from dpm_solver_amd import _lib as L  # noqa: E402
from dpm_solver_amd.launch_list import _FastRun  # noqa: E402

R, STEPS, SHAPE = 32, 20, (256, 4, 64, 64)
DTYPES = {"fp16": (torch.float16, L.DTYPE_F16), "fp32": (torch.float32, L.DTYPE_F32)}


def build(dev, dtype):
    td, code = DTYPES[dtype]
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: x, ns), ns, algorithm_type="dpmsolver++", state_dtype=td)
    plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N, unipc="bh2")
    forms = [st.form for st in plan.stages]
    assert forms == [L.FORM_LIN1] + [L.FORM_UNIPC] * (STEPS - 1), forms
    g = torch.Generator(device=dev).manual_seed(0)
    keep, recs = [plan], []      # recs[r][i] = (Stage, Buffers) of request r at stage i
    for r in range(R):
        fr = _FastRun(dpm, plan, SHAPE, td, dev, False)
        x_T = torch.randn(SHAPE, generator=g, device=dev).to(td)
        eps = (0.5 * torch.randn(SHAPE, generator=g, device=dev)).to(td)
        out = torch.empty(SHAPE, dtype=td, device=dev)
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


def positions(mode, k):
    return [k % STEPS if mode == "a" else (k + (STEPS * r) // R) % STEPS for r in range(R)]


def ticks_of(mode, recs):
    """the STEPS distinct ticks of a mode: (stage records, buffer records); request 0's options carry the mode's flags"""
    out, keep = [], []
    for k in range(STEPS):
        pos = positions(mode, k)
        sts = (L.Stage * R)(*[recs[r][pos[r]][0] for r in range(R)])
        bufs = (L.Buffers * R)(*[recs[r][pos[r]][1] for r in range(R)])
        if mode != "a":
            o = L.LaunchOpts()
            o.per_request_stages = 1
            o.no_fuse = 1 if mode == "c" else 0
            bufs[0].opts = C.pointer(o)
            keep.append(o)
        out.append((sts, bufs))
    return out, keep


def run(mode, recs, warmup, ticks, stream):
    tk, keep = ticks_of(mode, recs)

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
    return dict(mode=mode, ticks=ticks, us_per_request_stage=sec * 1e6 / (ticks * R), us_per_tick=sec * 1e6 / ticks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp16")
    ap.add_argument("--modes", default="abcL", help="a b c: lockstep, staggered, staggered request by request; L: unipc_stage.py")
    ap.add_argument("--ticks", type=int, default=200, help="a multiple of 20: every request passes every stage equally often")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3, help="rounds over the modes (alternating)")
    ap.add_argument("--label", default="", help="copied into the result (which library / commit this is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unipc_pool.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, recs = build(dev, a.dtype) if any(m in "abc" for m in a.modes) else (None, None)
    lock = None
    if "L" in a.modes:
        import unipc_stage as US
        plans, steady, rbs, keep_l = US.build(dev, a.dtype, R)
        US.run(plans, steady, rbs, R, "unipc2", stream)        # warm-up
        lock = lambda: dict(mode="L", us_per_request_stage=US.run(plans, steady, rbs, R, "unipc2", stream))
    rows = [lock() if m == "L" else run(m, recs, a.warmup, a.ticks, stream) for _ in range(a.repeat) for m in a.modes]
    res = {"workload": "32 x [256,4,64,64] %s, UniPC-2 bh2, 20 steps, frozen eps" % a.dtype, "label": a.label,
           "device": torch.cuda.get_device_name(0), "library": os.path.relpath(L.LIB_PATH, ROOT),
           "version": int(L.lib.dpm_version()), "ticks": a.ticks, "warmup": a.warmup, "repeat": a.repeat, "rows": rows}
    for m in a.modes:
        v = [r["us_per_request_stage"] for r in rows if r["mode"] == m]
        res[m] = dict(us_per_request_stage_median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")
    del keep


if __name__ == "__main__":
    main()
