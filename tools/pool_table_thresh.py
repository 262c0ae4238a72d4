#!/usr/bin/env python3
"""Many small thresholded requests in flight: what a stage tick of R single-image requests of a pixel-space model costs as ONE
table thresholding launch.

tools/pool_table_sde.py's method on DPM-Solver++(2M) plans of a solver with correcting_x0_fn="dynamic_thresholding": R (default
256) requests `[1,3,64,64]` -- 12288 elements, the largest sample a thresholded row holds --, 20 steps, order 2, request r at
stage (k + 20 r / R) mod 20 of tick k, frozen network output; the rows live in slabs, `--sets` (8) sets in rotation so that
every tick's inputs come from HBM.  Modes:

    H  DPM_TABLE_LAUNCH | DPM_TABLE_THRESH alone, on device tables filled and copied beforehand: the one stage_thresh_kernel_table launch
    h  FILL + the pinned host-to-device copy + LAUNCH, both with DPM_TABLE_THRESH: the whole stage side of a thresholding slab pool's tick
    a  the same arrays WITHOUT the flag (table_mode 0, per-request stages: what version 209 runs): R stage_thresh_kernel launches,
       each a cluster of six workgroups with the workspace of its own that it needs
    b  ONE lockstep thresholded launch of `[R,3,64,64]`, the same bytes at one stage: what the rows would cost if they marched in step

HIP events around `--ticks` back-to-back ticks after `--warmup` (mode a: a tenth of either, it is two orders slower),
`--repeat` rounds over the modes, alternating.  `--side S` (default 64) makes the samples `[3,S,S]`: smaller rows, for what the
per-sample LDS size buys.

    python tools/pool_table_thresh.py --dtype fp16 --out DIR/events.jsonl
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np
import torch

import pool_table as T
import dpm_solver_amd as D
from dpm_solver_amd import _lib as L

STEPS = T.STEPS
THRESH = L.TABLE_THRESH


def solver(td):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    return D.DPM_Solver(D.model_wrapper(lambda x, t: x, ns), ns, algorithm_type="dpmsolver++", state_dtype=td,
                        correcting_x0_fn="dynamic_thresholding")


class ThrSlabs:
    """`sets` sets of slabs [R, 3, 64, 64]: state in, state out, frozen eps, three cached model values; one zeroed
    thresholding workspace per row (mode a) and one for the lockstep launch (mode b)"""

    def __init__(self, dev, dtype, R, sets, side=64):
        SHAPE = (3, side, side)
        PER = self.per = 3 * side * side
        self.td, self.code = T.DTYPES[dtype]
        self.R, self.dev = R, dev
        dpm = solver(self.td)
        plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                             lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / dpm.noise_schedule.total_N)
        self.stages = [dpm._prep_stage(st.copy()) for st in plan.stages]
        assert all(st.flags & L.F_THRESH for st in self.stages)
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e=mk(0.5), out=torch.empty((R,) + SHAPE, dtype=self.td, device=dev), h=[mk(), mk(), mk()])
                     for _ in range(sets)]
        self.rowb = PER * torch.empty((), dtype=self.td).element_size()
        self.wsb = int(L.lib.dpm_threshold_workspace_bytes(1, PER))
        self.ws = torch.zeros(max(R * self.wsb, 16), dtype=torch.uint8, device=dev)
        self.ws_lone = torch.zeros(max(int(L.lib.dpm_threshold_workspace_bytes(R, PER)), 16), dtype=torch.uint8, device=dev)

    def buffers(self, S, r, st, n=None, batch=1):
        n = self.per if n is None else n
        b = L.Buffers()
        off = r * self.rowb
        b.x, b.e0, b.x_out = S["x"].data_ptr() + off, S["e"].data_ptr() + off, S["out"].data_ptr() + off
        if st.h1_slot >= 0:
            b.h1 = S["h"][st.h1_slot].data_ptr() + off
        if st.h2_slot >= 0:
            b.h2 = S["h"][st.h2_slot].data_ptr() + off
        if st.flags & L.F_STORE_M:
            b.m_out = S["h"][st.m_slot].data_ptr() + off
        b.n, b.batch, b.state_dtype, b.eps_dtype = n, batch, self.code, self.code
        return b

    def ticks(self):
        """the distinct ticks: (stages, buffers, options, host table, device table, R, request 0's own workspace)"""
        R = self.R
        out = []
        for k in range(max(STEPS, len(self.sets))):
            S = self.sets[k % len(self.sets)]
            pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
            sts = (L.Stage * R)(*[self.stages[p] for p in pos])
            bufs = (L.Buffers * R)(*[self.buffers(S, r, self.stages[pos[r]]) for r in range(R)])
            for r in range(R):
                bufs[r].workspace = self.ws.data_ptr() + r * self.wsb
            o = L.LaunchOpts()
            o.per_request_stages = 1
            bufs[0].opts = C.pointer(o)
            nb = L.table_bytes(R, THRESH)
            host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
            out.append((sts, bufs, o, host, torch.empty(nb, dtype=torch.uint8, device=self.dev), R, self.ws.data_ptr()))
        return out

    def lone(self):
        out = []
        for k in range(max(STEPS, len(self.sets))):
            st = self.stages[k % STEPS]
            b = self.buffers(self.sets[k % len(self.sets)], 0, st, n=self.R * self.per, batch=self.R)
            b.workspace = self.ws_lone.data_ptr()
            out.append((st, b))
        return out


def prefill(ticks, stream):
    for sts, bufs, o, host, dev, R, ws0 in ticks:
        o.table_mode, bufs[0].workspace = L.TABLE_FILL | THRESH, host.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        dev.copy_(host)
        o.table_mode, bufs[0].workspace = 0, ws0
    torch.cuda.synchronize()


def run(mode, ticks, lone, warmup, n_ticks, stream):
    if mode == "a":
        warmup, n_ticks = max(2, warmup // 10), max(5, n_ticks // 10)

    def tick(k):
        if mode == "b":
            st, b = lone[k % len(lone)]
            L.check(L.lib.dpm_stage_launch(C.byref(st), C.byref(b), stream))
            return
        sts, bufs, o, host, dev, R, ws0 = ticks[k % len(ticks)]
        if mode == "a":
            T._call(L.lib, sts, bufs, R, stream)
            return
        if mode == "h":
            o.table_mode, bufs[0].workspace = L.TABLE_FILL | THRESH, host.data_ptr()
            T._call(L.lib, sts, bufs, R, stream)
            dev.copy_(host, non_blocking=True)
        o.table_mode, bufs[0].workspace = L.TABLE_LAUNCH | THRESH, dev.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        o.table_mode, bufs[0].workspace = 0, ws0
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(T.DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--modes", default="Hhab")
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table_thresh.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,3,%d,%d] %s, 2M + dynamic thresholding, 20 steps, staggered, frozen eps, %d slab sets"
                       % (a.requests, a.side, a.side, a.dtype, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks}
    slabs = ThrSlabs(dev, a.dtype, a.requests, a.sets, a.side)
    ticks, lone = slabs.ticks(), slabs.lone()
    prefill(ticks, stream)
    rows = []
    for _ in range(a.repeat):
        for m in a.modes:
            rows.append(dict(mode=m, requests=a.requests, **run(m, ticks, lone, a.warmup, a.ticks, stream)))
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
