#!/usr/bin/env python3
"""Many small Perp-Neg requests in flight: what a stage tick of R single-image requests under Perp-Neg guidance (cfg_perp_neg:
the negative prompt's direction taken perpendicular to the positive one's, per image) costs as ONE table Perp-Neg launch.

tools/pool_table_pair.py's method on DPM-Solver++(2M) plans of a solver built on `cfg_perp_neg(model_fn, n, 1.0)` at guidance
scale 7.5: R (default 256) requests `[1,4,64,64]`, 20 steps, order 2, request r at stage (k + 20 r / R) mod 20 of tick k, frozen
network outputs (positive, empty, negative); the rows live in slabs as a perp_neg=True slab pool lays them out (the two duplicate
stores of a stage go to rows R + r and 2R + r of the [3R, ...] output slab), `--sets` (8) sets in rotation so that every tick's
inputs come from HBM.  Modes:

    H  DPM_TABLE_LAUNCH | DPM_TABLE_PERP alone, on device tables filled and copied beforehand: the one stage_perp_kernel_table
       launch, both duplicate stores included
    h  FILL + the pinned host-to-device copy + LAUNCH, both with DPM_TABLE_PERP: the whole stage side of a Perp-Neg slab pool's
       tick
    a  the same rows in a mode-0 per-request-stage call, without the copies (the lone kernel has no second store): R
       stage_perp_kernel launches of one workgroup each -- what a tick cost before the row kind existed
    b  ONE lockstep stage_perp_kernel launch of `[R,4,64,64]`: the same inputs at one stage, one store of the state
    c  mode b plus the `torch.cat([x] * 3)` that builds the network's next input from its result: what a caller pays for the
       bytes mode H moves
    P  the two-condition table tick of the same rows (cfg_pair, DPM_TABLE_PAIR: the same three outputs and three stores, no
       per-sample pass), one stage_pair_kernel_table launch
    Z  the CFG-Zero* table tick of the same rows (DPM_TABLE_ZSTAR: a per-sample pass over two outputs, two stores), one
       stage_zstar_kernel_table launch

HIP events around `--ticks` back-to-back ticks after `--warmup` (mode a: a tenth of either, it is two orders slower),
`--repeat` rounds over the modes, alternating.  `--wall`: host time per tick of a Perp-Neg slab pool of R rows against a
RequestPool of the same requests (one network call per request).

    python tools/pool_table_perp.py --dtype fp16 --out DIR/events.jsonl
    python tools/pool_table_perp.py --wall
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np
import torch

import pool_table as T
import pool_table_pair as TP
import dpm_solver_amd as D
from dpm_solver_amd import _lib as L

STEPS, SHAPE, PER = T.STEPS, T.SHAPE, T.PER
PERP = L.TABLE_PERP
SCALE, NEG_SCALE = 7.5, 1.0
FLAG = {"perp": PERP, "pair": L.TABLE_PAIR, "zstar": L.TABLE_ZSTAR}


def solver(td, kind="perp", net=lambda x, t, c: x):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=SCALE, condition=torch.ones(1),
                         unconditional_condition=torch.zeros(1))
    fn = {"perp": lambda: D.cfg_perp_neg(fn, torch.full((1,), 0.5), NEG_SCALE),
          "pair": lambda: D.cfg_pair(fn, torch.full((1,), 0.5), TP.SCALE2, nested=True),
          "zstar": lambda: D.cfg_zero_star(fn)}[kind]()
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", state_dtype=td)


class PerpSlabs(TP.PairSlabs):
    """PairSlabs' sets of slabs; the stage records of the rows under `cfg_perp_neg` (`stages`), and under `cfg_pair` and
    `cfg_zero_star` for the comparison ticks (`other`)"""

    def __init__(self, dev, dtype, R, sets):
        self.td, self.code = T.DTYPES[dtype]
        self.R, self.dev = R, dev
        self.other = {}
        for kind in ("perp", "pair", "zstar"):
            dpm = solver(self.td, kind)
            plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                                 lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / dpm.noise_schedule.total_N)
            self.other[kind] = [dpm._prep_stage(st.copy()) for st in plan.stages]
        self.stages = self.other["perp"]
        two = L.GUIDE["classifier-free-2"]
        assert all(st.guidance == two and st.flags & L.F_CFG2_PERP and st.cg_scale == NEG_SCALE for st in self.stages)
        assert all(st.guidance == two and not st.flags & L.F_CFG2_PERP for st in self.other["pair"])
        assert all(st.flags & L.F_CFG_ZSTAR for st in self.other["zstar"])
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e0=mk(0.5), e1=mk(0.5), e2=mk(0.5), out=torch.empty((3 * R,) + SHAPE, dtype=self.td, device=dev),
                          h=[mk(), mk(), mk()]) for _ in range(sets)]
        self.rowb = PER * torch.empty((), dtype=self.td).element_size()

    def ticks(self, kind="perp", copies=True):
        """the distinct ticks of the rows under `kind`: (stages, buffers, options, host table, device table, R);
        copies=False: the rows as their lone launches take them"""
        R, stages = self.R, self.other[kind]
        out = []
        for k in range(max(STEPS, len(self.sets))):
            S = self.sets[k % len(self.sets)]
            pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
            sts = (L.Stage * R)(*[stages[p] for p in pos])
            bufs = (L.Buffers * R)(*[self.buffers(S, r, stages[pos[r]], copies=copies) for r in range(R)])
            o = L.LaunchOpts()
            o.per_request_stages = 1
            bufs[0].opts = C.pointer(o)
            nb = L.table_bytes(R, FLAG[kind])
            host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
            out.append((sts, bufs, o, host, torch.empty(nb, dtype=torch.uint8, device=self.dev), R))
        return out


def prefill(ticks, stream, flag=PERP):
    TP.prefill(ticks, stream, flag)


def run(mode, ticks, lone, warmup, n_ticks, stream, pair=None, zstar=None, nocopy=None):
    """pair / zstar: the ticks of modes P / Z (PerpSlabs.ticks("pair") / ("zstar"), prefilled with their flags); nocopy: those of
    mode a (PerpSlabs.ticks(copies=False))"""
    if mode == "a":
        warmup, n_ticks = max(2, warmup // 10), max(5, n_ticks // 10)
    flag = {"P": FLAG["pair"], "Z": FLAG["zstar"]}.get(mode, PERP)

    def tick(k):
        if mode in "bc":
            st, b, x = lone[k % len(lone)]
            L.check(L.lib.dpm_stage_launch(C.byref(st), C.byref(b), stream))
            if mode == "c":
                torch.cat([x] * 3)
            return
        sts, bufs, o, host, dev, R = (pair if mode == "P" else zstar if mode == "Z" else nocopy if mode == "a" else ticks)[k % len(ticks)]
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


def wall(dev, dtype, R, ticks):
    """host wall time per tick, steady state: a SlabPool(perp_neg=True) of R rows, every request with a guidance scale and a
    negative scale of its own (three each, in rotation), against a RequestPool of the same requests under the wrapper's scales
    -- one network call per request and one lone stage_perp_kernel launch per request inside the tick's call"""
    def dpm(td):
        return solver(td, net=lambda x, t, c: x * 0.5)

    def own(n):
        return dict(guidance_scale=(1.5, 3.0, SCALE)[n % 3], neg_scale=(0.5, NEG_SCALE, 2.0)[n // 3 % 3])
    return T.wall(dev, dtype, R, ticks, {"slab_perp": lambda td, g: (dpm(td).request_pool(slots=R, perp_neg=True), own),
                                         "request_pool": lambda td, g: (dpm(td).request_pool(), T.no_kwargs)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(T.DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--modes", default="HhabcPZ")
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table_perp.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,4,64,64] %s, 2M + cfg_perp_neg(7.5, 1.0), 20 steps, staggered, frozen outputs, %d slab sets"
                       % (a.requests, a.dtype, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks,
           "dtype": a.dtype}
    if a.wall:
        res["wall"] = wall(dev, a.dtype, a.requests, min(a.ticks, 200))
    else:
        slabs = PerpSlabs(dev, a.dtype, a.requests, a.sets)
        ticks, lone, nocopy = slabs.ticks(), slabs.lone(), slabs.ticks(copies=False)
        pair, zstar = slabs.ticks("pair"), slabs.ticks("zstar")
        prefill(ticks, stream)
        prefill(pair, stream, FLAG["pair"])
        prefill(zstar, stream, FLAG["zstar"])
        rows = []
        for _ in range(a.repeat):
            for m in a.modes:
                rows.append(dict(mode=m, requests=a.requests, **run(m, ticks, lone, a.warmup, a.ticks, stream, pair, zstar, nocopy)))
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
