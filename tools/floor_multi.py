#!/usr/bin/env python3
"""The FLOOR of the fused 32-request 2M launch (the bench's headline kernel, stage_kernel_multi at 32 x [256,4,64,64] fp16).

`dpm_floor_multi_launch` (lab build) moves the fused launch's five streams per request -- three reads, two writes, 8 MiB each,
1.34 GB per launch -- with no arithmetic, in the fused kernel's 4 KiB tiles and XCD split, over

    load path      global_load_dwordx4 into registers | LDS-DMA (global_load_lds_dwordx4 into the wavefront's own rows)
    nt             on the loads; on the d store and on the e store separately (else write-through, the product's store)
    grid           one-shot workgroups (the product's shape) | resident grid of 2 / 4 / 8 workgroups per CU, each workgroup a
                   contiguous run of its XCD's tiles or strided over them
    pipe           1 or 2 tiles of loads in flight per wavefront (the next tile's loads issued before this tile's stores)

Launches run back to back like bench.py's: launch k reads x_k, eps, m_k and writes x_k+1, m_k+1 (three x and two m buffers
per request in rotation), so that every input was last written one launch (1.3 GB of other traffic) earlier.  In the same
process and trace the product's fused kernel runs bench.py's workload (dpm_plan_run_multi, 32 requests, frozen eps) before
and after the sweep.

    python tools/floor_multi.py --check                                     # every variant writes d = a ^ b, e = b ^ c
    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python tools/floor_multi.py --trace-only --seq DIR/seq.json
    python tools/floor_multi.py --summarise DIR --seq DIR/seq.json --out profiles/...json
"""
import argparse
import ctypes as C
import glob
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

R, NBYTES = 32, 256 * 4 * 64 * 64 * 2          # 32 requests, 8 MiB per stream and request
PEAK = 8000.0                                   # GB/s
ALG = 5 * R * NBYTES                            # bytes per launch


def cfg_id(c):
    return "p%d_nt%d_pi%d_g%d_i%d" % (c["load_path"], c["nt"], c["pipe"], c["blocks_per_cu"], c["interleave"])


def all_configs():
    out = []
    for path, nt, pipe, (bpc, ilv) in itertools.product((0, 1), range(8), (1, 2), ((0, 0), (2, 0), (2, 1), (4, 0), (4, 1), (8, 0), (8, 1))):
        out.append(dict(load_path=path, nt=nt, pipe=pipe, blocks_per_cu=bpc, interleave=ilv))
    return out


def desc(L, c):
    f = L.FloorMultiDesc()
    for k, v in c.items():
        setattr(f, k, v)
    return f


class Streams:
    """per request: 3 x buffers, 2 m buffers, eps -- rotated launch by launch like bench.py's trajectory"""

    def __init__(self, torch, dev, n_req, nbytes):
        n = nbytes // 4
        g = torch.Generator(device="cpu").manual_seed(99)
        mk = lambda: torch.randint(0, 2 ** 31 - 1, (n,), dtype=torch.int32, generator=g).to(dev)
        self.X = [[mk() for _ in range(3)] for _ in range(n_req)]
        self.H = [[mk() for _ in range(2)] for _ in range(n_req)]
        self.E = [mk() for _ in range(n_req)]
        self.n_req, self.nbytes = n_req, nbytes

    def tables(self, k):
        P = C.c_void_p * self.n_req
        a = P(*[self.X[r][k % 3].data_ptr() for r in range(self.n_req)])
        b = P(*[self.E[r].data_ptr() for r in range(self.n_req)])
        c = P(*[self.H[r][k % 2].data_ptr() for r in range(self.n_req)])
        d = P(*[self.X[r][(k + 1) % 3].data_ptr() for r in range(self.n_req)])
        e = P(*[self.H[r][(k + 1) % 2].data_ptr() for r in range(self.n_req)])
        return a, b, c, d, e

    def launch(self, L, f, k, stream):
        a, b, c, d, e = self.tables(k)
        L.check(L.lib.dpm_floor_multi_launch(C.byref(f), a, b, c, d, e, self.n_req, self.nbytes, stream, None))


def check():
    """every variant writes d = a ^ b and e = b ^ c: 7 requests of 13 tiles (a tile count that is no multiple of the XCD
    split or of any grid) and the full 32 x 8 MiB shape"""
    import _lab  # noqa: F401
    import torch
    from dpm_solver_amd import _lib as L
    L.require_lab("tools/floor_multi.py")
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = n = 0
    for n_req, nbytes, cfgs in ((7, 13 * 4096, all_configs()), (R, NBYTES, all_configs()[::9])):
        s = Streams(torch, dev, n_req, nbytes)
        for cf in cfgs:
            for r in range(n_req):
                s.X[r][1].zero_()
                s.H[r][1].zero_()
            s.launch(L, desc(L, cf), 0, stream)
            torch.cuda.synchronize()
            ok = all(torch.equal(s.X[r][1], s.X[r][0] ^ s.E[r]) and torch.equal(s.H[r][1], s.E[r] ^ s.H[r][0]) for r in range(n_req))
            n += 1
            if not ok:
                bad += 1
                print("WRONG", cfg_id(cf), n_req, nbytes)
        del s
        torch.cuda.empty_cache()
    print("floor_multi variants checked: %d launches, %d wrong" % (n, bad))
    return bad == 0


def trace_only(args):
    """the product's fused launches (bench.py's workload) / every floor configuration, `--launches` back to back each, twice
    (forward, then reverse order) / the product again.  The order goes to --seq for --summarise."""
    import _lab  # noqa: F401
    import torch
    import bench
    import dpm_solver_amd as D
    from dpm_solver_amd import _lib as L
    L.require_lab("tools/floor_multi.py")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    sptr = C.c_void_p(stream.cuda_stream)
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(bench.sd_alphas_cumprod()))
    dpm = D.DPM_Solver(D.model_wrapper(lambda x, t: x, ns), ns, algorithm_type="dpmsolver++", state_dtype=torch.float16)
    plan = dpm._get_plan(method="multistep", order=2, steps=bench.STEPS_SOLVER, skip_type="time_uniform",
                         solver_type="dpmsolver", lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N)
    sets = bench.make_sets(R, torch.float16, dev, seed=1234)
    rbs = (L.RunBuffers * R)(*[s_["rb"] for s_ in sets])
    resm = (C.c_int * R)()
    s = Streams(torch, dev, R, NBYTES)
    seq = []

    def product(tag):
        for _ in range(args.trajectories):
            L.check(L.lib.dpm_plan_run_multi(plan.handle, rbs, R, sptr, None, resm))
        seq.append(dict(id=tag, product=True, trajectories=args.trajectories))
    cfgs = all_configs() if not args.configs else [c for c in all_configs() if cfg_id(c) in args.configs.split(",")]
    product("product_before")
    k = 0
    for rep, order in enumerate((cfgs, cfgs[::-1])):
        for cf in order:
            f = desc(L, cf)
            for _ in range(args.launches):
                s.launch(L, f, k, sptr)
                k += 1
            seq.append(dict(id=cfg_id(cf), product=False, launches=args.launches, rep=rep))
    product("product_after")
    torch.cuda.synchronize()
    json.dump(seq, open(args.seq, "w"))
    print("traced %d floor configurations x 2, %d floor launches" % (len(cfgs), k))


def summarise(args):
    f = sorted(glob.glob(os.path.join(args.summarise, "**", "*kernel_trace.csv"), recursive=True))
    assert f, "no *kernel_trace.csv under %s" % args.summarise
    import csv
    rows = []
    for fn in f:
        with open(fn) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    names = [r[2] for r in rows]
    du = np.array([(r[1] - r[0]) / 1e3 for r in rows])
    floor_rows = [i for i, n in enumerate(names) if "floor_multi_kernel" in n]
    two = [i for i, n in enumerate(names) if "stage_kernel_multi<__half, __half, 1," in n]   # FORM_TWO: 18 of 20 stages
    seq = json.load(open(args.seq))
    skip = args.warmup
    per_cfg, pos = {}, 0
    for s in seq:
        if s["product"]:
            continue
        n = s["launches"]
        per_cfg.setdefault(s["id"], []).extend(du[floor_rows[pos + skip:pos + n]].tolist())
        pos += n
    assert pos == len(floor_rows), (pos, len(floor_rows))
    # product rows: before / after the sweep by position relative to the floor rows
    first_floor = floor_rows[0] if floor_rows else len(rows)
    before = du[[i for i in two if i < first_floor]]
    after = du[[i for i in two if i > first_floor]]

    def st(v):
        v = np.asarray(v)
        return dict(mean_us=round(float(v.mean()), 2), median_us=round(float(np.median(v)), 2),
                    p10_us=round(float(np.percentile(v, 10)), 2), p90_us=round(float(np.percentile(v, 90)), 2), rows=int(v.size),
                    tb_per_s=round(ALG / float(v.mean()) / 1e6, 3))
    res = dict(what="rocprofv3 --kernel-trace rows, launches back to back: 32 x [256,4,64,64] fp16 2M stage, %d B per launch "
                    "(3 reads + 2 writes); floor = dpm_floor_multi_launch (no arithmetic), product = stage_kernel_multi FORM_TWO "
                    "under dpm_plan_run_multi (bench.py's workload)" % ALG,
               product_before=st(before), product_after=st(after), floor={k: st(v) for k, v in per_cfg.items()})
    prod = float(np.concatenate([before, after]).mean())
    ranked = sorted(res["floor"].items(), key=lambda kv: kv[1]["mean_us"])
    res["product_mean_us"] = round(prod, 2)
    res["best_floor"] = dict(id=ranked[0][0], **ranked[0][1], headroom=round(1 - ranked[0][1]["mean_us"] / prod, 4))
    res["ranked"] = [(k, v["mean_us"]) for k, v in ranked]
    print(json.dumps({k: v for k, v in res.items() if k not in ("floor", "ranked")}, indent=1))
    for k, v in ranked[:25]:
        print("  %-24s %8.2f us  %.3f TB/s  (%d rows)" % (k, v["mean_us"], v["tb_per_s"], v["rows"]))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--configs", default="")
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trajectories", type=int, default=4)
    ap.add_argument("--seq", default="floor_multi_seq.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args)
    if args.check:
        sys.exit(0 if check() else 1)
    if args.trace_only:
        return trace_only(args)
    ap.print_help()


if __name__ == "__main__":
    main()
