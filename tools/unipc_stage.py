#!/usr/bin/env python3
"""The steady UniPC-2 stage against the third-order multistep `++` stage (MS3): the same four read and two write streams,
the same shape, the same slot of the same loop.  R requests of [256,4,64,64] advanced stage by stage by dpm_plan_run_multi
(frozen network outputs; with R = 32 every stage's inputs come from HBM: the other requests' 1.3 GB passed through the
Infinity Cache in between), kernel-only durations by the HIP events the library brackets its launches with.  The two plans
alternate inside one process; per repeat the mean over the steady stages (UniPC: second-order corrector + second-order
predictor; MS3: form MS3) in microseconds per request-stage.  Product library.

    python tools/unipc_stage.py --dtype fp16 --requests 32 --repeats 7 [--json OUT]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/unipc_stage.py --dtype fp16 --repeats 3
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(dev, dtype, requests, steps=20):
    """(plans, stage selectors, run buffers, tensors to keep alive) for the UniPC-2 and the 3M `++` plan"""
    import torch
    import bench
    import dpm_solver_amd as D
    from dpm_solver_amd import _lib as L
    dt = bench._DT[dtype]
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(bench.sd_alphas_cumprod()))
    dpm = D.DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver++")
    kw = dict(method="multistep", steps=steps, skip_type="time_uniform", solver_type="dpmsolver", lower_order_final=False,
              denoise_to_zero=False, t_T=1.0, t_0=1e-3)
    plans = {"unipc2": dpm._get_plan(order=2, unipc="bh2", **kw), "ms3": dpm._get_plan(order=3, **kw)}
    both = L.F_UNIPC_DP | L.F_UNIPC_P2
    steady = {"unipc2": [i for i, s in enumerate(plans["unipc2"].stages) if s.form == L.FORM_UNIPC and s.flags & both == both],
              "ms3": [i for i, s in enumerate(plans["ms3"].stages) if s.form == L.FORM_MS3]}
    shape = (bench.B,) + bench.SHAPE
    code = {torch.float32: L.DTYPE_F32, torch.float16: L.DTYPE_F16, torch.bfloat16: L.DTYPE_BF16}[dt]
    g = torch.Generator().manual_seed(4321)
    keep, rbs = [], (L.RunBuffers * requests)()
    for r in range(requests):
        ts = [torch.randn(shape, generator=g).to(dev, dt)] + [torch.empty(shape, device=dev, dtype=dt) for _ in range(6)]
        e0 = (0.1 * torch.randn(shape, generator=g)).to(dev, dt)
        keep.append((ts, e0))
        rb = rbs[r]
        for i in range(4):
            rb.xbuf[i] = ts[i].data_ptr()
        for i in range(3):
            rb.hist[i] = ts[4 + i].data_ptr()
        rb.e0 = e0.data_ptr()
        rb.n, rb.batch = ts[0].numel(), shape[0]
        rb.state_dtype = rb.eps_dtype = code
    return plans, steady, rbs, keep


def run(plans, steady, rbs, requests, which, stream):
    """one trajectory of every request through plan `which`: mean kernel-only us per request-stage over its steady stages"""
    from dpm_solver_amd import _lib as L
    ns_ = len(plans[which].stages)
    ms = (C.c_float * (requests * ns_))()
    L.check(L.lib.dpm_plan_run_multi(plans[which].handle, rbs, requests, stream, ms, None))
    vals = [ms[r * ns_ + i] * 1e3 for r in range(requests) for i in steady[which]]
    return sum(vals) / len(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32", "bf16"])
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    plans, steady, rbs, keep = build(dev, args.dtype, args.requests)
    for w in ("unipc2", "ms3"):                              # warm-up: first-launch costs
        run(plans, steady, rbs, args.requests, w, stream)
    rows = {"unipc2": [], "ms3": []}
    for _ in range(args.repeats):                            # alternating: both see the same box state
        for w in ("ms3", "unipc2"):
            rows[w].append(run(plans, steady, rbs, args.requests, w, stream))
    out = {"dtype": args.dtype, "requests": args.requests, "shape": [256, 4, 64, 64], "us_per_request_stage": rows,
           "ratio_of_medians": sorted(rows["unipc2"])[len(rows["unipc2"]) // 2] / sorted(rows["ms3"])[len(rows["ms3"]) // 2],
           "ms3_spread": max(rows["ms3"]) / min(rows["ms3"]), "unipc2_spread": max(rows["unipc2"]) / min(rows["unipc2"])}
    print(json.dumps(out))
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
