#!/usr/bin/env python3
"""The SDE 2M stage against the ODE 2M stage in the same situation: DPM_Solver.sample() and .sample_sde() (20 steps, order 2)
on one [256,4,64,64] request with a random-init torch network (bench.LoopNet) between the stages, so that every stage's
inputs come from HBM.  Product library; meant to run under the profiler, the stage-kernel rows then summarised:

    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/sde_stage.py --dtype fp16
    python tools/in_loop.py --summarise DIR/kt --pattern stage_kernel
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32", "bf16"])
    ap.add_argument("--kind", default="gemm")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--trajectories", type=int, default=6)
    args = ap.parse_args()
    import torch
    import bench
    import dpm_solver_amd as D
    dev = torch.device("cuda", 0)
    dtype = bench._DT[args.dtype]
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(bench.sd_alphas_cumprod()))
    net = bench.LoopNet(args.kind, args.width, dtype, dev)
    x_T = torch.randn((bench.B,) + bench.SHAPE, generator=torch.Generator().manual_seed(4321)).to(dev, dtype)
    dpm = D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++", state_dtype=dtype)
    with torch.no_grad():
        for i in range(args.trajectories):       # alternating: the two samplers see the same network and the same box state
            ode = dpm.sample(x_T, steps=20, order=2)
            sde = dpm.sample_sde(x_T, steps=20, order=2, seed=i)
        torch.cuda.synchronize()
    assert torch.isfinite(ode.float()).all() and torch.isfinite(sde.float()).all()
    print("done: %d ODE + %d SDE trajectories of [%d,4,64,64] %s" % (args.trajectories, args.trajectories, bench.B, args.dtype))


if __name__ == "__main__":
    main()
