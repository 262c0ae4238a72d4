"""The host-side plan of a thresholded launch (csrc/dpm_thresh_plan.hpp: thr_launch_plan -- cluster shape, fp32 quantile rank,
top-K front-end test, one-hop quota and slot geometry, workspace stride, range error) pinned without a GPU: a stand-alone
driver (tests/thr_plan_driver.cpp, plain g++, the header alone) runs the case table of tests/golden/thr_plan_cases.json and
every numeric field is compared with the values recorded there.  The recorded values were produced by the arithmetic block of
launch_thresh as it stood BEFORE the plan was hoisted out of it (copied verbatim into a scratch harness), not by
thr_launch_plan.  A wrong slot_shift or mrank does not fail on the GPU -- the kernel falls back to its general route with the
same bits and more time -- so this is where such a slip shows."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "thr_plan_cases.json")))
IN_KEYS = ("batch", "per_sample", "thr_ratio", "thr_max", "n_cu", "cluster_in_graph", "cluster_one_hop", "capturing", "vec",
           "fastdiv")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """the driver's answer to every case of the table: one compile, one run"""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("thr_plan") / "thr_plan_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "dpm_solver_amd", "csrc"), os.path.join(ROOT, "tests", "thr_plan_driver.cpp"),
                    "-o", exe], check=True)
    text = "".join(" ".join(str(c["in"][k]) for k in IN_KEYS) + "\n" for c in CASES)
    out = subprocess.run([exe], input=text, check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(out) == len(CASES)
    return [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in line.split()} for line in out]


def _find(plans, **want):
    hits = [p for c, p in zip(CASES, plans) if all(c["in"][k] == v for k, v in want.items())]
    assert len(hits) == 1, want
    return hits[0]


def test_the_header_needs_nothing_of_hip():
    src = open(os.path.join(ROOT, "dpm_solver_amd", "csrc", "dpm_thresh_plan.hpp")).read()
    incs = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert all(i.startswith("<") and "hip" not in i for i in incs if i != '"dpm_hip.h"'), incs


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "%d_%s" % (i, CASES[i]["note"].replace(" ", "_") or "plain"))
def test_every_field_matches_the_recorded_plan(plans, i):
    want, got = CASES[i]["out"], plans[i]
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, "%s: (got, recorded) %s" % (CASES[i]["in"], diff)


def test_the_table_covers_what_it_is_meant_to(plans):
    """the properties the cases were chosen for, stated independently of the recorded numbers"""
    base = dict(thr_ratio="0.995", n_cu=256, cluster_one_hop=1)
    cfg5 = _find(plans, batch=32, per_sample=12288, capturing=0, **base)
    assert cfg5["k"] == 6 and cfg5["topk"] == 63 and cfg5["quota"] > 0
    assert _find(plans, batch=32, per_sample=12288, capturing=1, cluster_in_graph=0, **base)["k"] == 1
    assert _find(plans, batch=32, per_sample=12288, capturing=1, cluster_in_graph=1, **base)["k"] == 6
    big, big_cap = (_find(plans, batch=64, per_sample=196608, capturing=c, **base) for c in (0, 1))
    assert big["k"] == 16 and big_cap == big                       # no cluster-free shape: keeps its cluster under capture
    assert _find(plans, batch=512, per_sample=12288, **base)["k"] == 1      # kfill = 1
    tiny = _find(plans, batch=1, per_sample=7, **base)
    assert tiny["vec"] == 0 and tiny["k"] == 1 and tiny["chunk"] == 8
    assert _find(plans, batch=8, per_sample=2050, **base)["chunk"] == 2052   # rounded up to whole 4-element groups
    mid = _find(plans, thr_ratio="0.5")
    assert mid["topk"] == 0 and mid["quota"] == 0
    assert _find(plans, cluster_one_hop=0)["quota"] == 0
    two = _find(plans, cluster_one_hop=2)
    assert two["quota"] == cfg5["quota"] and two["debug_reject"] == 1
    assert _find(plans, n_cu=64)["k"] == 4
    errs = [p for p in plans if p["err"]]
    assert len(errs) == 2 and all(not any(v for k, v in p.items() if k != "err") for p in errs)
    for p in plans:
        if not p["err"]:
            assert p["slot_cap"] == (1 << p["slot_shift"] if p["quota"] else 0) and p["tp_k"] == p["k"] and p["tp_chunk"] == p["chunk"]
