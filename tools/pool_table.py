#!/usr/bin/env python3
"""Many small requests in flight: what a stage tick of R single-image requests costs as ONE table launch and as R / 16 launches.

Workload: R (default 256) DPM-Solver++(2M) requests `[1,4,64,64]`, 20 steps, request r at stage (k + 20 r / R) mod 20 of tick k,
frozen network output (the ticks measure the stage side alone).  The rows live in slabs, as in a SlabPool; `--sets` (8) sets of
slabs are used in rotation -- 8 x 42 MB in fp16, more than the Infinity Cache -- so every tick's inputs come from HBM, as they do
when a network ran in between.  Modes, all through dpm_stage_launch_multi with per-request stage records on the SAME arrays:

    T  DPM_TABLE_LAUNCH alone, on device tables filled and copied beforehand: the one stage_kernel_table launch
    t  DPM_TABLE_FILL + the pinned host-to-device copy + DPM_TABLE_LAUNCH: the whole stage side of a slab pool's tick
    0  table_mode = 0 on this library: R / 16 stage_kernel_het launches (the code every commit before version 208 runs)
    p  the same call on ANOTHER build of the library (--parent-lib: the parent commit's libdpm_hip.so), in the same process
    l  for scale: ONE dpm_stage_launch of [R,4,64,64] on the same slabs -- the same bytes as one lockstep request

HIP events around `--ticks` back-to-back ticks after `--warmup`, `--repeat` rounds over the modes, alternating.  `--wall` times
whole pool ticks on the host instead (perf_counter around step(), a cheap elementwise network): a SlabPool of R rows against a
RequestPool of the same R requests.

    python tools/pool_table.py --dtype fp16 --parent-lib PATH --out DIR/events.jsonl
    python tools/pool_table.py --sweep 17,24,32,48,64,128,256          # table against het launches by group size
    python tools/pool_table.py --wall
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dpm_solver_amd as D  # noqa: E402
from dpm_solver_amd import _lib as L  # noqa: E402

STEPS, SHAPE = 20, (4, 64, 64)
PER = 4 * 64 * 64
DTYPES = {"fp16": (torch.float16, L.DTYPE_F16), "fp32": (torch.float32, L.DTYPE_F32)}


def solver(td, net=lambda x, t: x):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    return D.DPM_Solver(D.model_wrapper(net, ns), ns, algorithm_type="dpmsolver++", state_dtype=td)


class Slabs:
    """`sets` sets of slabs [R, 4, 64, 64]: state in, state out, frozen eps, three cached model values"""

    def __init__(self, dev, dtype, R, sets):
        self.td, self.code = DTYPES[dtype]
        self.R, self.dev = R, dev
        dpm = solver(self.td)
        self.plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                                  lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / dpm.noise_schedule.total_N)
        self.stages = [dpm._prep_stage(st.copy()) for st in self.plan.stages]
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e=mk(0.5), out=torch.empty((R,) + SHAPE, dtype=self.td, device=dev), h=[mk(), mk(), mk()])
                     for _ in range(sets)]
        self.rowb = PER * torch.empty((), dtype=self.td).element_size()

    def buffers(self, S, r, st, n=PER, batch=1):
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

    def ticks(self, count=None):
        """the distinct ticks (one per set and position offset): (stages, buffers, options, host table, device table)"""
        R = count or self.R
        out = []
        for k in range(max(STEPS, len(self.sets))):
            S = self.sets[k % len(self.sets)]
            pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
            sts = (L.Stage * R)(*[self.stages[p] for p in pos])
            bufs = (L.Buffers * R)(*[self.buffers(S, r, self.stages[pos[r]]) for r in range(R)])
            o = L.LaunchOpts()
            o.per_request_stages = 1
            bufs[0].opts = C.pointer(o)
            nb = L.table_bytes(R)
            host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
            out.append((sts, bufs, o, host, torch.empty(nb, dtype=torch.uint8, device=self.dev), R))
        return out

    def lone(self):
        out = []
        for k in range(max(STEPS, len(self.sets))):
            st = self.stages[k % STEPS]
            out.append((st, self.buffers(self.sets[k % len(self.sets)], 0, st, n=self.R * PER, batch=self.R)))
        return out


def _call(lib, sts, bufs, R, stream):
    rc = lib.dpm_stage_launch_multi(sts, bufs, R, stream)
    if rc:
        raise RuntimeError("dpm_stage_launch_multi: %d %s" % (rc, lib.dpm_last_error()))


def prefill(ticks, stream):
    for sts, bufs, o, host, dev, R in ticks:
        o.table_mode, bufs[0].workspace = L.TABLE_FILL, host.data_ptr()
        _call(L.lib, sts, bufs, R, stream)
        dev.copy_(host)
        o.table_mode, bufs[0].workspace = 0, None
    torch.cuda.synchronize()


def run(mode, ticks, lone, warmup, n_ticks, stream, parent=None):
    def tick(k):
        if mode == "l":
            st, b = lone[k % len(lone)]
            L.check(L.lib.dpm_stage_launch(C.byref(st), C.byref(b), stream))
            return
        sts, bufs, o, host, dev, R = ticks[k % len(ticks)]
        if mode == "T":
            o.table_mode, bufs[0].workspace = L.TABLE_LAUNCH, dev.data_ptr()
            _call(L.lib, sts, bufs, R, stream)
        elif mode == "t":
            o.table_mode, bufs[0].workspace = L.TABLE_FILL, host.data_ptr()
            _call(L.lib, sts, bufs, R, stream)
            dev.copy_(host, non_blocking=True)
            o.table_mode, bufs[0].workspace = L.TABLE_LAUNCH, dev.data_ptr()
            _call(L.lib, sts, bufs, R, stream)
        else:
            o.table_mode, bufs[0].workspace = 0, None
            _call(parent if mode == "p" else L.lib, sts, bufs, R, stream)
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


def wall(dev, dtype, R, ticks, pools):
    """host wall time per tick, steady state, of each of `pools`: name -> make.  make(td, g) returns the pool and the function
    kwargs(n) of what `submit` gets for request n beside its x_T, steps and order (it may draw what they need from the generator
    g).  R / 20 requests are submitted per tick: as many finish as arrive."""
    td = DTYPES[dtype][0]
    out = {}
    for name, make in pools.items():
        g = torch.Generator(device=dev).manual_seed(1)
        xs = [torch.randn((1,) + SHAPE, generator=g, device=dev).to(td) for _ in range(R)]
        pool, kwargs = make(td, g)
        nxt = 0
        per = max(1, R // STEPS)

        def feed():
            nonlocal nxt
            for _ in range(per):
                pool.submit(xs[nxt % R], steps=STEPS, order=2, **kwargs(nxt))
                nxt += 1
        for _ in range(STEPS + 2):          # fill: R / 20 requests per tick, then steady state
            feed()
            pool.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ticks):
            feed()
            pool.step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out[name] = dict(ticks=ticks, active=len(pool), host_us_per_tick=(t1 - t0) * 1e6 / ticks,
                         wall_us_per_tick=(t2 - t0) * 1e6 / ticks)
        del pool
    return out


def wall_solver(td):
    """the solver of the --wall pools: a cheap elementwise network"""
    return solver(td, net=lambda x, t: x * 0.5)


def no_kwargs(n):
    return {}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--modes", default="Tt0l")
    ap.add_argument("--parent-lib", default=None, help="another build of libdpm_hip.so for mode p (adds it to --modes)")
    ap.add_argument("--ticks", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweep", default=None, help="comma-separated group sizes: modes T and 0 at each")
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,4,64,64] %s, 2M, 20 steps, staggered, frozen eps, %d slab sets" % (a.requests, a.dtype, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks}
    if a.wall:
        res["wall"] = wall(dev, a.dtype, a.requests, min(a.ticks, 400), {
            "slab": lambda td, g: (wall_solver(td).request_pool(slots=a.requests), no_kwargs),
            "request_pool": lambda td, g: (wall_solver(td).request_pool(), no_kwargs)})
    else:
        slabs = Slabs(dev, a.dtype, a.requests, a.sets)
        parent, modes = None, a.modes
        if a.parent_lib:
            parent = C.CDLL(a.parent_lib)
            parent.dpm_stage_launch_multi.argtypes = L.lib.dpm_stage_launch_multi.argtypes
            parent.dpm_last_error.restype = C.c_char_p
            res["parent_version"] = int(parent.dpm_version())
            modes += "p"
        sizes = [int(v) for v in a.sweep.split(",")] if a.sweep else [a.requests]
        lone = slabs.lone()
        rows = []
        for size in sizes:
            ticks = slabs.ticks(size)
            if size > 16:
                prefill(ticks, stream)
            for _ in range(a.repeat):
                for m in (("T0" if size > 16 else "0") if a.sweep else modes):
                    rows.append(dict(mode=m, requests=size, **run(m, ticks, lone, a.warmup, a.ticks, stream, parent)))
            del ticks
        res["rows"] = rows
        for size in sizes:
            for m in sorted({r["mode"] for r in rows}):
                v = [r["us_per_tick"] for r in rows if r["mode"] == m and r["requests"] == size]
                if v:
                    res["%s@%d" % (m, size)] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
