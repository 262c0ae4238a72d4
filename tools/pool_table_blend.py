#!/usr/bin/env python3
"""Many small inpainting requests in flight: what a stage tick of R single-image DPM_F_BLEND requests costs as ONE table blend launch.

tools/pool_table.py's workload and method with a mask blend on every stage: R (default 256) requests `[1,4,64,64]`, 20 steps,
order 2, request r at stage (k + 20 r / R) mod 20 of tick k, frozen network output, each row with its own known image and noise
(slabs next to the state slabs) and a mask of its own -- full size, or `[H,W]` (`--mask hw`); `--sets` (8) sets in rotation so
that every tick's inputs come from HBM.  Modes, all through dpm_stage_launch_multi with per-request stage records:

    B  DPM_TABLE_LAUNCH | DPM_TABLE_BLEND alone, on device tables filled and copied beforehand: the one stage_kernel_table_blend launch
    b  FILL + the pinned host-to-device copy + LAUNCH, both with DPM_TABLE_BLEND: the whole stage side of an inpainting slab tick
    2  DPM_TABLE_LAUNCH WITHOUT the flag on the same arrays: R lone DPM_F_BLEND launches (what version 210 runs)
    T  the ODE tick of the same rows of the same slabs: the one stage_kernel_table launch, for the blend's price

HIP events around `--ticks` back-to-back ticks after `--warmup`, `--repeat` rounds over the modes, alternating.  `--wall` times
whole pool ticks on the host instead: a SlabPool(inpaint=True) of R inpainting rows against a plain SlabPool of R rows.

    python tools/pool_table_blend.py --dtype fp16 --out DIR/events.jsonl
    python tools/pool_table_blend.py --wall
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np
import torch

import dpm_solver_amd as D
import pool_table as T
from dpm_solver_amd import _lib as L

STEPS, SHAPE, PER = T.STEPS, T.SHAPE, T.PER
BLEND = L.TABLE_BLEND


class BlendSlabs(T.Slabs):
    """pool_table.Slabs with a mask, a known-image and a noise slab per set and DPM_F_BLEND on every stage"""

    def __init__(self, dev, dtype, R, sets, mask="full"):
        super().__init__(dev, dtype, R, sets)
        self.ode_stages = self.stages
        self.stages = []
        for st in self.ode_stages:
            s = st.copy()
            s.flags |= L.F_BLEND
            s.blend_alpha, s.blend_sigma = st.alpha_e, st.sigma_e
            self.stages.append(s)
        g = torch.Generator(device=dev).manual_seed(1)
        self.period = PER if mask == "full" else SHAPE[1] * SHAPE[2]
        for S in self.sets:
            S["mask"] = (torch.rand((R, self.period), generator=g, device=dev) > 0.5).to(self.td)
            S["a"] = torch.randn((R,) + SHAPE, generator=g, device=dev).to(self.td)
            S["b"] = torch.randn((R,) + SHAPE, generator=g, device=dev).to(self.td)

    def ticks(self, count=None, blend=True):
        """the distinct ticks: (stages, buffers, options, host table, device table, R)"""
        R = count or self.R
        stages = self.stages if blend else self.ode_stages
        es = self.rowb // PER
        out = []
        for k in range(max(STEPS, len(self.sets))):
            S = self.sets[k % len(self.sets)]
            pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
            sts = (L.Stage * R)(*[stages[p] for p in pos])
            bufs = (L.Buffers * R)(*[self.buffers(S, r, stages[pos[r]]) for r in range(R)])
            for r in range(R if blend else 0):
                b = bufs[r]
                b.mask, b.mask_period = S["mask"].data_ptr() + r * self.period * es, self.period
                b.blend_a, b.blend_b = S["a"].data_ptr() + r * self.rowb, S["b"].data_ptr() + r * self.rowb
            o = L.LaunchOpts()
            o.per_request_stages = 1
            bufs[0].opts = C.pointer(o)
            nb = L.table_bytes(R, BLEND)
            host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
            out.append((sts, bufs, o, host, torch.empty(nb, dtype=torch.uint8, device=self.dev), R))
        return out


def prefill(ticks, flag, stream):
    for sts, bufs, o, host, dev, R in ticks:
        o.table_mode, bufs[0].workspace = L.TABLE_FILL | flag, host.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        dev.copy_(host)
        o.table_mode, bufs[0].workspace = 0, None
    torch.cuda.synchronize()


def run(mode, ticks, ode_ticks, warmup, n_ticks, stream):
    def tick(k):
        sts, bufs, o, host, dev, R = (ode_ticks if mode == "T" else ticks)[k % len(ticks)]
        flag = BLEND if mode in "Bb" else 0
        if mode == "b":
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


def wall(dev, dtype, R, ticks, mask):
    """host wall time per tick, steady state: a SlabPool(inpaint=True) of R inpainting rows against a plain SlabPool of R rows"""
    def inpaint(td, g):
        dpm = T.wall_solver(td)
        mk = lambda: torch.randn((1,) + SHAPE, generator=g, device=dev).to(td)
        mshape = SHAPE if mask == "full" else SHAPE[1:]
        mbs = [D.MaskBlend(dpm.noise_schedule, (torch.rand(mshape, generator=g, device=dev) > 0.5).to(td), x0=mk(), noise=mk())
               for _ in range(R)]
        return dpm.request_pool(slots=R, inpaint=True), lambda n: dict(blend=mbs[n % R])
    return T.wall(dev, dtype, R, ticks, {
        "slab_inpaint": inpaint, "slab_plain": lambda td, g: (T.wall_solver(td).request_pool(slots=R), T.no_kwargs)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(T.DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--mask", choices=("full", "hw"), default="full")
    ap.add_argument("--modes", default="Bb2T")
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table_blend.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,4,64,64] %s, 2M + mask blend (%s mask), 20 steps, staggered, frozen eps, %d slab sets"
                       % (a.requests, a.dtype, a.mask, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks}
    if a.wall:
        res["wall"] = wall(dev, a.dtype, a.requests, min(a.ticks, 400), a.mask)
    else:
        slabs = BlendSlabs(dev, a.dtype, a.requests, a.sets, a.mask)
        ticks, ode_ticks = slabs.ticks(), slabs.ticks(blend=False)
        prefill(ticks, BLEND, stream)
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
