#!/usr/bin/env python3
"""What guidance rescale costs per stage inside a torch network loop, by rocprofv3 rows (profiles/r21_cfg_rescale.md).

Three routes to a classifier-free stage, in the same process, the same loop and the same slot between two network calls:
  (a) torch    the only route before DPM_F_CFG_RESCALE: an "uncond" wrapper around a torch model that does torch.cat([x] * 2),
               the network, the classifier-free blend and diffusers' rescale_noise_cfg, then the plain stage kernel
  (b) cfg      the flag-less classifier-free stage kernel of the same shape (no rescale at all): the floor
  (c) fused    cfg_rescale(model_fn, phi): stage_rescale_kernel
Every network call is bracketed by a sentinel kernel (a fill of one int64 element), so the rows between the sentinel behind
call i and the sentinel in front of call i + 1 are the solver side of stage i, whatever kernels that takes.

    rocprofv3 --kernel-trace -d DIR -o kt -- python tools/rescale_in_loop.py --run --manifest DIR/manifest.json
    python tools/rescale_in_loop.py --summarise DIR --manifest DIR/manifest.json [--md profiles/r21_cfg_rescale.md]
"""
import argparse
import glob
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((8, 4, 64, 64), "float32"), ((8, 4, 64, 64), "float16"), ((64, 4, 64, 64), "float32"), ((64, 4, 64, 64), "float16"),
         ((8, 4, 128, 128), "float32")]            # (shape, state dtype); the network answers in fp16 everywhere
ROUTES = ("torch", "cfg", "fused")
STEPS, TRAJ, WARM, ROUNDS = 10, 12, 3, 2
PHI, SCALE = 0.7, 7.5
SENTINEL = "FillFunctor"


def run(manifest_path):
    import numpy as np
    import torch
    import bench
    import dpm_solver_amd as D

    dev = torch.device("cuda:0")
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    net = bench.LoopNet(kind="conv", width=64, dtype=torch.float16, device=dev)
    sent = torch.zeros(1, dtype=torch.int64, device=dev)
    manifest = []

    def network(x, t, c=None):
        sent.fill_(0)
        out = net(x.half(), t)
        sent.fill_(0)
        return out

    def torch_route(x, t):
        out = network(torch.cat([x] * 2), torch.cat([t] * 2))
        e1, e0 = out.chunk(2)
        g = e1 + SCALE * (e0 - e1)
        axes = list(range(1, g.ndim))
        r = g * (e0.std(dim=axes, keepdim=True) / g.std(dim=axes, keepdim=True))
        return PHI * r + (1 - PHI) * g

    def solver(route, sdt):
        skw = dict(state_dtype=sdt) if sdt is torch.float16 else {}
        if route == "torch":
            return D.DPM_Solver(D.model_wrapper(torch_route, ns), ns, **skw)
        c = torch.ones(1, device=dev)
        fn = D.model_wrapper(network, ns, guidance_type="classifier-free", guidance_scale=SCALE, condition=c,
                             unconditional_condition=c * 0)
        return D.DPM_Solver(D.cfg_rescale(fn, PHI) if route == "fused" else fn, ns, **skw)

    for shape, sdn in CASES:
        sdt = getattr(torch, sdn)
        x = torch.randn(shape, generator=torch.Generator().manual_seed(0)).to(dev, sdt)
        solvers = {r: solver(r, sdt) for r in ROUTES}
        for rnd in range(ROUNDS + 1):                     # round 0 warms every route up
            for route in ROUTES:
                n = WARM if rnd == 0 else TRAJ
                for _ in range(n):
                    solvers[route].sample(x, steps=STEPS, order=2)
                torch.cuda.synchronize()
                manifest.append(dict(shape=list(shape), state=sdn, route=route, warm=rnd == 0, trajectories=n, calls=n * STEPS))
    with open(manifest_path, "w") as f:
        json.dump(dict(steps=STEPS, sentinel=SENTINEL, blocks=manifest), f)
    print("manifest: %d blocks -> %s" % (len(manifest), manifest_path))


def summarise(d, manifest_path, md=None):
    import numpy as np
    f = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
    assert f, "no *_results.db under %s" % d
    cur = sqlite3.connect(f[0]).cursor()
    rows = cur.execute("select name, start, duration from kernels order by start").fetchall()
    man = json.load(open(manifest_path))
    is_sent = [man["sentinel"] in r[0] and ("long" in r[0] or "Il" in r[0]) for r in rows]
    pos = [i for i, s in enumerate(is_sent) if s]
    n_calls = sum(b["calls"] for b in man["blocks"])
    assert len(pos) == 2 * n_calls + 1, "found %d sentinel rows, the manifest says %d network calls" % (len(pos), n_calls)
    pos = pos[1:]                                     # (the first fill is the sentinel tensor's own torch.zeros)
    stats, names = {}, {}
    call = 0
    for b in man["blocks"]:
        key = (tuple(b["shape"]), b["state"], b["route"])
        for j in range(b["calls"]):
            behind = pos[2 * (call + j) + 1]
            last_of_traj = (j + 1) % man["steps"] == 0
            if not b["warm"] and not last_of_traj:
                nxt = pos[2 * (call + j) + 2]
                seg = rows[behind + 1:nxt]
                busy = sum(r[2] for r in seg) / 1e3
                span = ((seg[-1][1] + seg[-1][2]) - seg[0][1]) / 1e3 if seg else 0.0
                stats.setdefault(key, []).append((busy, span, len(seg)))
                for r in seg:
                    names.setdefault(key, {}).setdefault(r[0][:120], []).append(r[2] / 1e3)
        call += b["calls"]
    out = ["| shape | state / network | route | stages | kernels per stage | busy us (median) | p10 | p90 | span us (median) |\n",
           "|---|---|---|---|---|---|---|---|---|\n"]
    med = {}
    for (shape, sdn, route), v in stats.items():
        a = np.array(v)
        med[(shape, sdn, route)] = float(np.median(a[:, 0]))
        out.append("| %s | %s / float16 | %s | %d | %.1f | %.2f | %.2f | %.2f | %.2f |\n" % (
            list(shape), sdn, route, len(v), a[:, 2].mean(), np.median(a[:, 0]), np.percentile(a[:, 0], 10),
            np.percentile(a[:, 0], 90), np.median(a[:, 1])))
    out.append("\n| shape | state | (c)/(a) busy | (c)/(b) busy |\n|---|---|---|---|\n")
    for shape, sdn in sorted({k[:2] for k in med}):
        a, b, c = (med.get((shape, sdn, r), float("nan")) for r in ROUTES)
        out.append("| %s | %s | %.3f | %.3f |\n" % (list(shape), sdn, c / a, c / b))
    out.append("\nkernels of the solver side, per route (median us, rows):\n\n")
    for key, ks in names.items():
        out.append("- %s %s %s: %s\n" % (list(key[0]), key[1], key[2], "; ".join(
            "`%s` %.2f x%d" % (n.replace("|", "/"), float(np.median(v)), len(v)) for n, v in sorted(ks.items(), key=lambda kv: -sum(kv[1]))[:8])))
    text = "".join(out)
    print(text)
    if md:
        with open(md, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--summarise")
    ap.add_argument("--manifest", required=True)
    ap.add_argument("--md")
    a = ap.parse_args()
    if a.run:
        run(a.manifest)
    else:
        summarise(a.summarise, a.manifest, a.md)
