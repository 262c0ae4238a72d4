#!/usr/bin/env python3
"""Many small SDE requests in flight: what a stage tick of R single-image SDE requests costs as ONE table noise launch.

tools/pool_table.py's workload and method with "DPM++ 2M SDE" plans: R (default 256) SDE-DPM-Solver++ requests `[1,4,64,64]`, 20
steps, order 2, request r at stage (k + 20 r / R) mod 20 of tick k, frozen network output, each request with a seed of its own
in a dpm_launch_opts of its own; the rows live in slabs, `--sets` (8) sets in rotation so that every tick's inputs come from HBM.
Modes, all through dpm_stage_launch_multi with per-request stage records:

    N  DPM_TABLE_LAUNCH | DPM_TABLE_NOISE alone, on device tables filled and copied beforehand: the one stage_kernel_table_noise launch
    n  FILL + the pinned host-to-device copy + LAUNCH, both with DPM_TABLE_NOISE: the whole stage side of an SDE slab pool's tick
    2  DPM_TABLE_LAUNCH WITHOUT the flag on the same arrays: R / 16 stage_kernel_het_noise launches (what version 208 runs)
    T  the ODE tick of the same rows of the same slabs (2M plans): the one stage_kernel_table launch, for the generator's price

HIP events around `--ticks` back-to-back ticks after `--warmup`, `--repeat` rounds over the modes, alternating.  `--wall` times
whole pool ticks on the host instead: a SlabPool(sde=True) of R rows against a RequestPool of the same R SDE requests.

    python tools/pool_table_sde.py --dtype fp16 --out DIR/events.jsonl
    python tools/pool_table_sde.py --wall
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np
import torch

import pool_table as T
from dpm_solver_amd import _lib as L

STEPS, SHAPE, PER = T.STEPS, T.SHAPE, T.PER
NOISE = L.TABLE_NOISE


class SdeSlabs(T.Slabs):
    """pool_table.Slabs with the stages of the SDE plan next to the ODE plan's (`ode_stages`)"""

    def __init__(self, dev, dtype, R, sets):
        super().__init__(dev, dtype, R, sets)
        dpm = T.solver(self.td)
        self.ode_stages = self.stages
        plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                             lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / dpm.noise_schedule.total_N, sde=True)
        self.stages = [dpm._prep_stage(st.copy()) for st in plan.stages]
        assert all(st.flags & L.F_NOISE for st in self.stages)

    def ticks(self, count=None, sde=True):
        """the distinct ticks: (stages, buffers, options, host table, device table, R, per-request options)"""
        R = count or self.R
        stages = self.stages if sde else self.ode_stages
        out = []
        for k in range(max(STEPS, len(self.sets))):
            S = self.sets[k % len(self.sets)]
            pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
            sts = (L.Stage * R)(*[stages[p] for p in pos])
            bufs = (L.Buffers * R)(*[self.buffers(S, r, stages[pos[r]]) for r in range(R)])
            own = [L.LaunchOpts() for _ in range(R)]
            for r, o in enumerate(own):
                o.noise_seed_lo, o.noise_seed_hi = 1000 + r, 7 * r
                bufs[r].opts = C.pointer(o)
            own[0].per_request_stages = 1
            nb = L.table_bytes(R, NOISE)
            host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
            out.append((sts, bufs, own[0], host, torch.empty(nb, dtype=torch.uint8, device=self.dev), R, own))
        return out


def prefill(ticks, flag, stream):
    for sts, bufs, o, host, dev, R, _ in ticks:
        o.table_mode, bufs[0].workspace = L.TABLE_FILL | flag, host.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        dev.copy_(host)
        o.table_mode, bufs[0].workspace = 0, None
    torch.cuda.synchronize()


def run(mode, ticks, ode_ticks, warmup, n_ticks, stream):
    def tick(k):
        sts, bufs, o, host, dev, R, _ = (ode_ticks if mode == "T" else ticks)[k % len(ticks)]
        flag = NOISE if mode in "Nn" else 0
        if mode == "n":
            o.table_mode, bufs[0].workspace = L.TABLE_FILL | flag, host.data_ptr()
            T._call(L.lib, sts, bufs, R, stream)
            dev.copy_(host, non_blocking=True)
        o.table_mode, bufs[0].workspace = L.TABLE_LAUNCH | flag, dev.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        o.table_mode, bufs[0].workspace = 0, None
    for k in range(warmup):
        tick(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(warmup, warmup + n_ticks):
        tick(k)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) / 1e3
    return dict(ticks=n_ticks, region_s=sec, us_per_tick=sec * 1e6 / n_ticks)


def wall(dev, dtype, R, ticks):
    """host wall time per tick, steady state: a SlabPool(sde=True) of R rows against a RequestPool of the same R SDE requests"""
    def sde_kwargs(n):
        return dict(sde=True, seed=n)
    return T.wall(dev, dtype, R, ticks, {
        "slab_sde": lambda td, g: (T.wall_solver(td).request_pool(slots=R, sde=True), sde_kwargs),
        "request_pool": lambda td, g: (T.wall_solver(td).request_pool(), sde_kwargs)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(T.DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--modes", default="Nn2T")
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table_sde.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,4,64,64] %s, 2M SDE, 20 steps, staggered, frozen eps, %d slab sets" % (a.requests, a.dtype, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks}
    if a.wall:
        res["wall"] = wall(dev, a.dtype, a.requests, min(a.ticks, 400))
    else:
        slabs = SdeSlabs(dev, a.dtype, a.requests, a.sets)
        ticks, ode_ticks = slabs.ticks(), slabs.ticks(sde=False)
        prefill(ticks, NOISE, stream)
        prefill(ode_ticks, 0, stream)
        rows = []
        for _ in range(a.repeat):
            for m in a.modes:
                rows.append(dict(mode=m, requests=a.requests, **run(m, ticks, ode_ticks, a.warmup, a.ticks, stream)))
        res["rows"] = rows
        for m in sorted({r["mode"] for r in rows}):
            v = [r["us_per_tick"] for r in rows if r["mode"] == m]
            res["%s@%d" % (m, a.requests)] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
