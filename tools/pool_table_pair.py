#!/usr/bin/env python3
"""Many small two-condition requests in flight: what a stage tick of R single-image requests under guidance over two conditions
(cfg_pair: InstructPix2Pix's image and text scales, composable conditions) costs as ONE table pair launch.

tools/pool_table_zstar.py's method on DPM-Solver++(2M) plans of a solver built on `cfg_pair(model_fn, c2, 1.5, nested=True)` at
guidance scale 7.5: R (default 256) requests `[1,4,64,64]`, 20 steps, order 2, request r at stage (k + 20 r / R) mod 20 of tick
k, frozen network outputs (condition, unconditional, second condition); the rows live in slabs as a pair=True slab pool lays them
out (the two duplicate stores of a stage go to rows R + r and 2R + r of the [3R, ...] output slab), `--sets` (8) sets in rotation
so that every tick's inputs come from HBM.  Modes:

    H  DPM_TABLE_LAUNCH | DPM_TABLE_PAIR alone, on device tables filled and copied beforehand: the one stage_pair_kernel_table
       launch, both duplicate stores included
    h  FILL + the pinned host-to-device copy + LAUNCH, both with DPM_TABLE_PAIR: the whole stage side of a pair slab pool's tick
    a  the same rows WITHOUT the flag and without the copies (the lone kernel has no second store): R stage_pair_kernel launches
    b  ONE lockstep stage_pair_kernel launch of `[R,4,64,64]`: the same inputs at one stage, one store of the state
    c  mode b plus the `torch.cat([x] * 3)` that builds the network's next input from its result: what a caller pays today for
       the bytes mode H moves
    p  the plain classifier-free table tick of the same rows (two outputs, one duplicate store), one stage_kernel_table launch

HIP events around `--ticks` back-to-back ticks after `--warmup` (mode a: a tenth of either, it is two orders slower),
`--repeat` rounds over the modes, alternating.

    python tools/pool_table_pair.py --dtype fp16 --out DIR/events.jsonl
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

STEPS, SHAPE, PER = T.STEPS, T.SHAPE, T.PER
PAIR = L.TABLE_PAIR
SCALE, SCALE2 = 7.5, 1.5


def solver(td, pair=True, net=lambda x, t, c: x):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=SCALE, condition=torch.ones(1),
                         unconditional_condition=torch.zeros(1))
    return D.DPM_Solver(D.cfg_pair(fn, torch.full((1,), 0.5), SCALE2, nested=True) if pair else fn, ns,
                        algorithm_type="dpmsolver++", state_dtype=td)


class PairSlabs:
    """`sets` sets of slabs: state in [R, 4, 64, 64], state out [3R, ...] (the two duplicate stores' thirds behind the first),
    the three frozen network outputs, three cached model values; the stage records of the rows under `cfg_pair` (`stages`) and
    under the bare classifier-free wrapper (`plain`)"""

    def __init__(self, dev, dtype, R, sets):
        self.td, self.code = T.DTYPES[dtype]
        self.R, self.dev = R, dev
        self.stages, self.plain = [], []
        for pair, into in ((True, self.stages), (False, self.plain)):
            dpm = solver(self.td, pair)
            plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                                 lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / dpm.noise_schedule.total_N)
            into += [dpm._prep_stage(st.copy()) for st in plan.stages]
        two = L.GUIDE["classifier-free-2"]
        assert all(st.guidance == two and st.cg_scale == SCALE2 - SCALE for st in self.stages)
        assert all(st.guidance == L.GUIDE["classifier-free"] for st in self.plain)
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e0=mk(0.5), e1=mk(0.5), e2=mk(0.5), out=torch.empty((3 * R,) + SHAPE, dtype=self.td, device=dev),
                          h=[mk(), mk(), mk()]) for _ in range(sets)]
        self.rowb = PER * torch.empty((), dtype=self.td).element_size()

    def buffers(self, S, r, st, n=PER, batch=1, copies=True):
        b = L.Buffers()
        off = r * self.rowb
        b.x, b.e0, b.e1 = S["x"].data_ptr() + off, S["e0"].data_ptr() + off, S["e1"].data_ptr() + off
        b.x_out = S["out"].data_ptr() + off
        if st.guidance == L.GUIDE["classifier-free-2"]:
            b.g = S["e2"].data_ptr() + off
            if copies:
                b.x_out2 = S["out"].data_ptr() + self.R * self.rowb + off
                b.thr_hint = S["out"].data_ptr() + 2 * self.R * self.rowb + off
        else:
            b.x_out2 = S["out"].data_ptr() + self.R * self.rowb + off
        if st.h1_slot >= 0:
            b.h1 = S["h"][st.h1_slot].data_ptr() + off
        if st.h2_slot >= 0:
            b.h2 = S["h"][st.h2_slot].data_ptr() + off
        if st.flags & L.F_STORE_M:
            b.m_out = S["h"][st.m_slot].data_ptr() + off
        b.n, b.batch, b.state_dtype, b.eps_dtype = n, batch, self.code, self.code
        return b

    def ticks(self, plain=False, copies=True):
        """the distinct ticks: (stages, buffers, options, host table, device table, R); plain: the same rows under classifier-free
        guidance; copies=False: the rows as their lone launches take them"""
        R, stages = self.R, self.plain if plain else self.stages
        out = []
        for k in range(max(STEPS, len(self.sets))):
            S = self.sets[k % len(self.sets)]
            pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
            sts = (L.Stage * R)(*[stages[p] for p in pos])
            bufs = (L.Buffers * R)(*[self.buffers(S, r, stages[pos[r]], copies=copies) for r in range(R)])
            o = L.LaunchOpts()
            o.per_request_stages = 1
            bufs[0].opts = C.pointer(o)
            nb = L.table_bytes(R, PAIR)
            host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
            out.append((sts, bufs, o, host, torch.empty(nb, dtype=torch.uint8, device=self.dev), R))
        return out

    def lone(self):
        """(stage, buffers, the [R, ...] result as a tensor): one lockstep launch per tick, no copies"""
        out = []
        for k in range(max(STEPS, len(self.sets))):
            st, S = self.stages[k % STEPS], self.sets[k % len(self.sets)]
            out.append((st, self.buffers(S, 0, st, n=self.R * PER, batch=self.R, copies=False), S["out"][:self.R]))
        return out


def prefill(ticks, stream, flag=PAIR):
    for sts, bufs, o, host, dev, R in ticks:
        o.table_mode, bufs[0].workspace = L.TABLE_FILL | flag, host.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        assert host[:16].view(torch.int32).tolist()[2:] == [R, 1], "the tick is not one run of rows"
        dev.copy_(host)
        o.table_mode, bufs[0].workspace = 0, None
    torch.cuda.synchronize()


def run(mode, ticks, lone, warmup, n_ticks, stream, plain=None, nocopy=None):
    """plain: the ticks of mode p (PairSlabs.ticks(plain=True), prefilled with flag 0); nocopy: those of mode a
    (PairSlabs.ticks(copies=False))"""
    if mode == "a":
        warmup, n_ticks = max(2, warmup // 10), max(5, n_ticks // 10)
    flag = 0 if mode in "pa" else PAIR

    def tick(k):
        if mode in "bc":
            st, b, x = lone[k % len(lone)]
            L.check(L.lib.dpm_stage_launch(C.byref(st), C.byref(b), stream))
            if mode == "c":
                torch.cat([x] * 3)
            return
        sts, bufs, o, host, dev, R = (plain if mode == "p" else nocopy if mode == "a" else ticks)[k % len(ticks)]
        if mode == "a":
            T._call(L.lib, sts, bufs, R, stream)
            return
        if mode == "h":
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(T.DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--modes", default="Hhabcp")
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table_pair.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,4,64,64] %s, 2M + cfg_pair(7.5, 1.5, nested), 20 steps, staggered, frozen outputs, %d slab sets"
                       % (a.requests, a.dtype, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks,
           "dtype": a.dtype}
    slabs = PairSlabs(dev, a.dtype, a.requests, a.sets)
    ticks, lone, plain, nocopy = slabs.ticks(), slabs.lone(), slabs.ticks(plain=True), slabs.ticks(copies=False)
    prefill(ticks, stream)
    prefill(plain, stream, flag=0)
    rows = []
    for _ in range(a.repeat):
        for m in a.modes:
            rows.append(dict(mode=m, requests=a.requests, **run(m, ticks, lone, a.warmup, a.ticks, stream, plain, nocopy)))
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
