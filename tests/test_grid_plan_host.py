"""The launch-shape arithmetic of the single-request launchers (csrc/dpm_grid_plan.hpp: stream_grid's threads and workgroups, the
`big` test of launch_stream, scalar_grid's workgroups, the big_tiles test, the block caps of dpm_add_noise_launch and
dpm_blend_launch) pinned without a GPU: a stand-alone driver (tests/grid_plan_driver.cpp, plain g++, the header alone) runs the
case table of tests/golden/grid_plan_cases.json and every field is compared with the values recorded there.  The recorded values
were produced by the arithmetic as it stood in dpm_launch.hpp and dpm_kernels.hip BEFORE it was hoisted (copied verbatim into a
scratch harness), not by the hoisted functions.  The table holds, for 256, 304 and 64 CUs, every size the large-route sweep uses
(tests/test_gpu_large_routes.py) and the sizes one below, at and one above each gate."""
import json
import os

import pytest

import grid_plan as GP

ROOT = GP.ROOT
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "grid_plan_cases.json")))
T = GP.T


@pytest.fixture(scope="module")
def plans():
    """the driver's answer to every case of the table: one compile, one run"""
    return GP.ask([c["in"] for c in CASES])


def test_the_header_needs_nothing_of_hip():
    src = open(os.path.join(GP.CSRC, "dpm_grid_plan.hpp")).read()
    incs = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert incs and all(i.startswith("<") and "hip" not in i for i in incs), incs


def test_the_launch_layer_calls_the_header():
    """the arithmetic lives in one place: the launchers hold no second copy of a gate"""
    launch = open(os.path.join(GP.CSRC, "dpm_launch.hpp")).read()
    kernels = open(os.path.join(GP.CSRC, "dpm_kernels.hip")).read()
    for call in ("stream_grid_plan(", "stream_big(", "scalar_grid_blocks("):
        assert call in launch, call
    assert "lone_takes_fused_shape(" in kernels and kernels.count("aux_grid_blocks(") == 3
    assert "4 * (int64_t)n_cu" not in launch and "n_cu * 16" not in launch and "* 16;" not in kernels


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "%d_%s_cu%d" % (i, CASES[i]["note"].replace(" ", "_"), CASES[i]["in"]["n_cu"]))
def test_every_field_matches_the_recorded_plan(plans, i):
    want, got = CASES[i]["out"], plans[i]
    assert sorted(got) == sorted(want) == sorted(GP.OUT_KEYS)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, "%s: (got, recorded) %s" % (CASES[i]["in"], diff)


def _find(plans, **want):
    hits = [p for c, p in zip(CASES, plans) if all(c["in"][k] == v for k, v in want.items())]
    assert len(hits) == 1, want
    return hits[0]


@pytest.mark.parametrize("n_cu", [256, 304, 64])
def test_the_table_covers_what_it_is_meant_to(plans, n_cu):
    """the gates, stated here independently of the recorded numbers AND of the header (the one place outside the product that
    spells them out), each crossed from both sides in the table"""
    bpc, big = GP.product_tuning()
    base = dict(n_cu=n_cu, blocks_per_cu=bpc, block_threads=0, big_tiles=big)
    g = GP.gates(n_cu)
    assert g == dict(W=4 * n_cu, K=bpc * n_cu, S=16 * n_cu * 256, B=big, A=16 * n_cu)
    W, K, S, B, A = (g[k] for k in "WKSBA")
    lo, at, hi = (_find(plans, n=(W + d) * T, u=1, **base) for d in (-1, 0, 1))
    assert (lo["threads"], at["threads"], hi["threads"]) == (256, 512, 512) and (lo["big"], at["big"]) == (0, 1)
    assert lo["blocks"] == W - 1 and at["blocks"] == W // 2 and hi["blocks"] == W // 2 + 1
    lo, at = (_find(plans, n=(2 * W + d) * T, u=2, **base) for d in (-1, 0))
    assert (lo["threads"], lo["iters"], at["threads"], at["iters"]) == (512, W, 512, W)        # 2W - 1 tiles: W pairs already
    assert _find(plans, n=W * T, u=2, **base)["threads"] == 256                               # U = 2 at W tiles: W / 2 iterations
    at, hi = _find(plans, n=K * T, u=1, **base), _find(plans, n=K * T + 8, u=1, **base)
    assert at["iters"] == K == 2 * at["blocks"] and hi["iters"] == K + 1 and hi["blocks"] == at["blocks"]
    at, hi = _find(plans, n=2 * K * T, u=2, **base), _find(plans, n=(2 * K + 1) * T, u=2, **base)
    assert at["iters"] == K and hi["iters"] == K + 1 and hi["blocks"] == at["blocks"] == K // 2
    lo, at, hi = (_find(plans, n=S + d, u=1, **base) for d in (-1, 0, 1))
    assert lo["scalar_blocks"] == at["scalar_blocks"] == hi["scalar_blocks"] == S // 256
    assert _find(plans, n=S + 1, u=1, **base)["scalar_blocks"] * 256 < S + 1
    lo, at, hi = (_find(plans, n=(B + d) * T, u=1, **base) for d in (-1, 0, 1))
    assert (lo["fused"], at["fused"], hi["fused"]) == (0, 1, 1)
    assert _find(plans, n=(B - 1) * T + 8, u=1, **base)["fused"] == 1 and _find(plans, n=(B - 1) * T - 8, u=1, **base)["fused"] == 0
    assert _find(plans, n=(B + 1) * T, u=1, **dict(base, big_tiles=0))["fused"] == 0
    lo, at, hi = (_find(plans, n=A * 256 + d, u=1, **base) for d in (-1, 0, 1))
    assert lo["aux_blocks"] == at["aux_blocks"] == hi["aux_blocks"] == A
    at, hi = _find(plans, n=8 * A * 256, u=1, **base), _find(plans, n=8 * A * 256 + 8, u=1, **base)
    assert at["aux_vec_blocks"] == hi["aux_vec_blocks"] == A
    assert _find(plans, n=0, u=1, **base)["blocks"] == 1 and _find(plans, n=1, u=1, **base)["scalar_blocks"] == 1
    assert _find(plans, n=(W + 3) * T, **dict(base, block_threads=256))["threads"] == 256
    assert _find(plans, n=5 * T, **dict(base, block_threads=512))["blocks"] == 3


def test_the_table_holds_every_size_of_the_sweep():
    import test_gpu_large_routes as R
    for n_cu in (256, 304, 64):
        have = {(c["in"]["n"], c["in"]["u"]) for c in CASES if c["in"]["n_cu"] == n_cu and c["in"]["block_threads"] == 0}
        sz = R.sizes(n_cu)
        for sec in ("a", "a_split", "b", "e"):
            assert all((n, u) in have for _, n in sz[sec] for u in (1, 2)), (n_cu, sec)
        assert all((n, 1) in have for _, n, _ in sz["c"]) and all((n, 1) in have for k in ("f_vec", "f_scalar", "f_blend") for n in sz[k])
        assert all((b * per, 1) in have for b in sz["g_batch"] for per in sz["g_per"])
