"""The table of the large-route sweep (tests/test_gpu_large_routes.py) checked without a GPU, at 256 CUs: the numpy doubles of
every cell run and stay inside their payloads, and the coverage rule holds -- with every route taken from the host build of
csrc/dpm_grid_plan.hpp (tests/grid_plan.py), so that moving a gate in the launch layer fails here instead of leaving the GPU
sweep on the wrong side of it."""
import gc

import pytest

import grid_plan as GP
import guarded as G
import test_gpu_edges as E
import test_gpu_large_routes as R

CU = R.HOST_CU
T = G.T
PAIRS, PAIR_IDS = E.PAIRS, E.PAIR_IDS
BIG = 10 * 1000 * 1000                # above this many elements the doubles run for one variant only


def _routes(p):
    return [(c, R.expected_route(c, p, CU)) for c in R.table(CU, p)]


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_every_gate_is_crossed_from_both_sides_for_every_pair(p):
    g = GP.gates(CU)
    W, K, S = g["W"], g["K"], g["S"]
    rt = _routes(p)
    a = [(c, r) for c, r in rt if c.sec == "a" and r[0] == "vector" and not c.v.get("stride_batch")]
    # 512-thread workgroups: below and at W tiles, U = 1
    assert {r[1] for c, r in a if c.n == (W - 1) * T} == {256} and {r[1] for c, r in a if c.n == W * T} == {512}
    assert any(r[1] == 512 and c.n == W * T + 8 for c, r in a)                       # an odd tile count under `sub`
    # the capped grid: one trip at K iterations, a second one 8 elements later, a third at 2K + 5 tiles
    assert {r[2] for c, r in a if c.n == K * T} == {1} and {r[2] for c, r in a if c.n == K * T + 8} == {2}
    assert {r[2] for c, r in a if c.tag == "2K+5"} == {3} and {r[2] for c, r in a if c.tag == "K+1r"} == {2}
    assert any(c.n % 8 for c, r in a if r[2] >= 2)                                   # loop plus ragged tail
    # the resident hot kernels: U = 1 at every small size, U = 2 from W tiles; 512 threads under U = 2 from 2W tiles; the cap
    b = [(c, r) for c, r in rt if c.sec == "b"]
    assert all(r[0] == "vector" for c, r in b)
    assert {r[3] for c, r in b if c.tag == "small"} == {1} and {r[3] for c, r in b if c.tag != "small"} == {2}
    assert {c.n for c, r in b if c.tag == "small"} == set(E.SIZES)
    assert {r[1] for c, r in b if c.tag == "W"} == {256} and {r[1] for c, r in b if c.tag == "2W"} == {512}
    assert {r[2] for c, r in b if c.tag == "2K"} == {1} and {r[2] for c, r in b if c.tag in ("2K+1", "2K+3r")} == {2}
    tiles = {c.tag: GP.route(c.n, CU)["iters"] for c, r in b}
    assert tiles["W+g"] % 2 == 1 and tiles["2K+1"] % 2 == 0                          # an odd tile count: the last pair's second tile is empty
    assert any(c.n % 8 for c, r in b if r[2] == 1 and c.tag != "small") and any(c.n % 8 for c, r in b if r[2] == 2)   # ragged under U = 2
    assert {v["form"] for c, r in b if r[2] == 2 for v in [c.v]} == {"LIN1", "TWO"}
    assert {c.v["store_m"] for c, r in b if r[2] == 2} == {True, False}
    # the one-element-per-lane kernels: at the cap, one element past it, a third trip; offset 1; a ragged mask blend
    c_ = [(c, r) for c, r in rt if c.sec == "c"]
    assert all(r[0] == "scalar" for c, r in c_)
    plain = [(c, r) for c, r in c_ if not c.v.get("stride_batch")]
    assert {r[2] for c, r in plain if c.n == S} == {1} and {r[2] for c, r in plain if c.n == S + 1} == {2}
    assert {r[2] for c, r in plain if c.tag == "2S+257"} == {3}
    assert {c.offset for c, r in c_ if r[2] >= 2} == {0, 1}
    for family, frag in (("unipc", "xc"), ("sde", "noise")):
        assert any(c.family == family and c.v.get(frag) and r[2] >= 2 for c, r in c_), family
    assert {c.v["form"] for c, r in c_ if r[2] >= 2} >= {"LIN1", "TWO", "MS3", "SS3T", "DENOISE", "UNIPC"}
    assert any(c.v["guidance"] == "classifier" and r[2] >= 2 for c, r in c_)
    assert any(c.v.get("sep_xe") and c.v["form"] == "TWO" and r[2] >= 2 for c, r in c_)
    assert any(c.v.get("stride_batch") == 2 and r[2] >= 2 for c, r in c_)
    assert any(c.v.get("blend") and E._blend_of(c.v, c.n)[0] % 8 and r[2] >= 2 for c, r in c_)


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_every_variant_is_met_on_a_looping_size(p):
    rt = _routes(p)
    loop = [(c, r) for c, r in rt if c.sec == "a" and r[2] >= 2]
    for family in ("kext", "unipc", "sde"):
        met = [c.v for c, r in loop if c.family == family]
        assert all(v in met for v in E.VARIANTS[family]), family
    kinds = {E._blend_of(c.v, R.n_of(c))[2] for c, r in loop if c.v.get("blend")}
    assert kinds == {"split", "pack", "ragged"}
    assert {c.v["stride_batch"] for c, r in loop if c.v.get("stride_batch")} == {2, 3}
    stream = [c.v for c, r in loop if c.family == "stream" and c.tag in ("K+g", "K+1r", "2K+5")]
    assert len(stream) == 9                                         # three looping sizes, three variants each
    assert {v["form"] for v in stream} == {"LIN1", "TWO", "MS3", "SS3T", "DENOISE"}
    assert {v["guidance"] for v in stream} == {"uncond", "classifier-free", "classifier"}
    assert {v["model"] for v in stream} == {"noise", "v"} and {v["store_m"] for v in stream} == {True, False}
    # the vector kernels among them loop too (a classifier-guided SS3T / DENOISE cell takes the one-element-per-lane kernel)
    assert sum(1 for c, r in loop if c.family == "stream" and r[0] == "vector") >= 6
    for family in ("kext", "unipc", "sde"):
        assert any(r[0] == "vector" and r[2] == 3 for c, r in loop if c.family == family), family


def test_the_other_sections_cross_their_gates():
    g = GP.gates(CU)
    B, A = g["B"], g["A"]
    sz = R.sizes(CU)
    e = [(tag, n, GP.route(n, CU)) for tag, n in sz["e"]]
    assert [r["fused"] for _, _, r in e] == [0, 1, 1] and e[0][2]["trips"] == 8 and e[2][1] % 8
    assert [R.edge_fused(n, v, CU) for tag, n, vt, v, p in R.edge_table(CU) if p == 3] == [
        False, False, False, True, True, False, False, False, False]
    assert {p for *_, p in R.edge_table(CU)} == {1, 3, 4}
    assert [GP.route(n, CU)["aux_vec_trips"] for n in sz["f_vec"]] == [1, 2, 3] and all(n % 8 == 0 for n in sz["f_vec"])
    assert [GP.route(n, CU)["aux_trips"] for n in sz["f_scalar"]] == [2, 3] and all(n % 8 for n in sz["f_scalar"])
    assert [GP.route(n, CU)["aux_trips"] for n in sz["f_blend"]] == [1, 2, 3]
    assert {off for *_, off in R.add_noise_cells(CU)} == {0, 1} and {nt for _, _, nt, _ in R.add_noise_cells(CU)} == {1, 3}
    assert sz["g_batch"] == [2 * CU + 1, 4 * CU + 3] and sz["g_per"] == [8, 257, 768]
    assert sz["g_clustered"][0] > CU and sz["g_clustered"][1] > 12288           # two workgroups per sample, at most CU clusters at once


@pytest.fixture(scope="module")
def cached_z():
    """the contract's z (sde_double.noise_z64) once per (seed, stage index), at the largest size of the table; every cell reads a
    prefix"""
    import numpy as np
    import sde_double as SD
    nz = max(R.n_of(c) for c in R.table(CU, 0) if c.v.get("noise"))
    cache, old = {}, SD.Z_SOURCE[0]

    def z(seed, index, n):
        if (seed, index) not in cache:
            cache[(seed, index)] = SD.noise_z64(seed, index, nz).astype(np.float32)
        assert n <= nz
        return cache[(seed, index)][:n]
    SD.Z_SOURCE[0] = z
    yield z
    SD.Z_SOURCE[0] = old


def _double(cell, p):
    case = R.make(cell, p)
    G.run_double(case)
    del case


PARTS = [("a", t) for t in R.A_TAGS] + [("b", t) for t in ("small", "large")] + [("c", "all")]


@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
@pytest.mark.parametrize("sec,tag", PARTS, ids=["%s-%s" % x for x in PARTS])
def test_the_doubles_of_every_cell_stay_inside_their_payloads(sec, tag, p, cached_z):
    """sizes above ten million elements (the eps_stride cells of the third-trip size): one variant"""
    mine = R._cells(sec, tag, p, CU) if sec == "a" else [c for c in R.table(CU, p) if c.sec == sec and (
        tag == "all" or (c.tag == "small") == (tag == "small"))]
    assert mine
    seen_big = set()
    for cell in mine:
        if R.n_of(cell) > BIG:
            if cell.tag in seen_big:
                continue
            seen_big.add(cell.tag)
        _double(cell, p)
    gc.collect()


def test_the_parts_are_the_table():
    for p in range(len(PAIRS)):
        cells = [c for t in R.A_TAGS for c in R._cells("a", t, p, CU)] + [c for c in R.table(CU, p) if c.sec in ("b", "c")]
        assert sorted(map(repr, cells)) == sorted(map(repr, R.table(CU, p)))
        assert [c for t in R.B_TAGS for c in R._cells("b", t, p, CU)] == [c for c in R.table(CU, p) if c.sec == "b"]
        assert [c for t in R.C_TAGS for c in R._cells("c", t, p, CU)] == [c for c in R.table(CU, p) if c.sec == "c"]


@pytest.mark.parametrize("p", R.E_PAIRS, ids=[PAIR_IDS[p] for p in R.E_PAIRS])
def test_the_doubles_of_the_big_tiles_edge(p):
    """above ten million elements: one variant per size"""
    for i, (tag, n) in enumerate(R.sizes(CU)["e"]):
        G.run_double(R.edge_case(n, R.EDGE[i][1], p))
        gc.collect()
