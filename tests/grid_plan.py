"""The launch-shape arithmetic of csrc/dpm_grid_plan.hpp asked from Python -- TEST INFRASTRUCTURE.

tests/grid_plan_driver.cpp (plain g++, the header alone) is compiled once per process; `ask` hands it rows and returns its
answers.  `gates(n_cu)` finds every size gate of the launch layer by scanning those answers -- nothing here restates a gate --
and `route(n, n_cu, ...)` says which launch shape a launch of n elements gets.  The product's tuning defaults the driver takes as
arguments (blocks per CU, big_tiles) are read from csrc/dpm_device.hpp."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpm_solver_amd", "csrc")
T = 2048
OUT_KEYS = ("iters", "threads", "blocks", "big", "scalar_blocks", "fused", "aux_vec_blocks", "aux_blocks")
IN_KEYS = ("n", "u", "n_cu", "blocks_per_cu", "block_threads", "big_tiles")


@functools.lru_cache(None)
def product_tuning():
    """(blocks_per_cu, big_tiles) of the product library: Tuning's defaults in csrc/dpm_device.hpp"""
    src = open(os.path.join(CSRC, "dpm_device.hpp")).read()
    bpc = re.search(r"int blocks_per_cu = (\d+);", src)
    big = re.search(r"#define DPM_BIG_TILES_DEFAULT (\d+)", src)
    assert bpc and big and "int big_tiles = DPM_BIG_TILES_DEFAULT;" in src
    return int(bpc.group(1)), int(big.group(1))


@functools.lru_cache(None)
def driver():
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    tmp = tempfile.mkdtemp(prefix="grid_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "grid_plan_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "grid_plan_driver.cpp"),
                    "-o", exe], check=True)
    return exe


def ask(rows):
    """rows of IN_KEYS (dicts) -> the driver's answers (dicts of OUT_KEYS)"""
    text = "".join(" ".join(str(int(r[k])) for k in IN_KEYS) + "\n" for r in rows)
    out = subprocess.run([driver()], input=text, check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(out) == len(rows)
    return [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in line.split()} for line in out]


def row(n, n_cu, u=1):
    bpc, big = product_tuning()
    return dict(n=n, u=u, n_cu=n_cu, blocks_per_cu=bpc, block_threads=0, big_tiles=big)


@functools.lru_cache(None)
def route(n, n_cu, u=1):
    """the product's launch shape of n elements at u tiles per iteration, and what follows from it: `trips` = loop trips of the
    busiest 256-lane group of the streaming vector kernels, `scalar_trips` / `aux_trips` / `aux_vec_trips` = of the busiest lane
    of the one-element-per-lane kernels and of add_noise / blend"""
    r = ask([row(n, n_cu, u)])[0]
    return _with_trips(r, n)


def _with_trips(r, n):
    r = dict(r)
    groups = r["blocks"] * (r["threads"] // 256)
    r["trips"] = -(-r["iters"] // groups)
    r["scalar_trips"] = -(-n // (256 * r["scalar_blocks"])) if n else 0
    r["aux_trips"] = -(-n // (256 * r["aux_blocks"])) if n else 0
    r["aux_vec_trips"] = -(-(n // 8) // (256 * r["aux_vec_blocks"])) if n >= 8 else 0
    return r


@functools.lru_cache(None)
def gates(n_cu):
    """every size gate of the launch layer at n_cu CUs, found on the driver's answers (one run):
      W  tiles from which a U = 1 launch has 512-thread workgroups (and the resident hot kernels take U = 2)
      K  most iterations a U = 1 launch runs in one trip (one more: a group loops)
      S  most elements the one-element-per-lane kernels run in one trip
      B  tiles from which a lone launch takes the fused shape
      A  most 256-thread workgroups of add_noise / blend (one more 256-element block: a lane loops)"""
    top = 70000
    ans = [_with_trips(a, t * T) for t, a in enumerate(ask([row(t * T, n_cu) for t in range(top)]))]
    w = next(t for t in range(1, top) if ans[t]["threads"] == 512)
    assert all(ans[t]["big"] == (t >= w) for t in range(top)), "the `big` test and the 512-thread test part ways"
    k = next(t for t in range(1, top) if ans[t]["trips"] > 1) - 1
    b = next(t for t in range(1, top) if ans[t]["fused"])
    el = [_with_trips(a, j * 256) for j, a in enumerate(ask([row(j * 256, n_cu) for j in range(top)]))]
    s = 256 * (next(j for j in range(1, top) if el[j]["scalar_trips"] > 1) - 1)
    a_ = next(j for j in range(1, top) if el[j]["aux_trips"] > 1) - 1
    assert a_ == next(j for j in range(1, top) if el[8 * j]["aux_vec_trips"] > 1) - 1, "add_noise's two routes are capped alike"
    return dict(W=w, K=k, S=s, B=b, A=a_)
