"""The tile space of a mixed-shape heterogeneous launch (csrc/dpm_het_shapes.hpp: het_shape_plan, het_shape_find,
het_virtual_tile -- the functions stage_kernel_shapes itself calls) pinned without a GPU: a stand-alone driver
(tests/het_shapes_driver.cpp, plain g++, the header alone) walks every case and this file compares what it prints with the
mapping written down here independently -- request-major super-tiles, U tiles of 2048 elements each.  A virtual index that
reached the wrong request, or a super-tile no workgroup reached, would on the GPU be a request advanced with another's
coefficients or left partly unwritten."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "dpm_solver_amd", "csrc", "dpm_het_shapes.hpp")
SIZES = [8, 2040, 2048, 2056, 4088, 4096, 4104, 6144, 6152, 8200, 16384]
COUNTS = [2, 3, 8, 9, 16]
HET_MAX = 16


def _cases():
    """(u, [n]): per count and U, the sizes in rotation from three starting points, descending, and two seeded draws"""
    rng, out = random.Random(207), []
    for u in (1, 2):
        for c in COUNTS:
            for start in (0, 3, 7):
                out.append((u, [SIZES[(start + r) % len(SIZES)] for r in range(c)]))
            out.append((u, [SIZES[-1 - r % len(SIZES)] for r in range(c)]))
            for _ in range(2):
                ns = [rng.choice(SIZES) for _ in range(c)]
                while len(set(ns)) < 2:             # (a mixed group has at least two sizes)
                    ns = [rng.choice(SIZES) for _ in range(c)]
                out.append((u, ns))
    return out


CASES = _cases()
UNIFORM = [(1, [4096] * 5), (2, [8] * 16)]
# no plan: too many members, an empty member, no member, 2^32 super-tiles
UNFIT = [(1, [2048] * 17), (2, [4096, 0, 8]), (1, []), (1, [(1 << 28) * 2048] * 16), (2, [(1 << 31) * 4096, 8])]
ALMOST = [(1, [((1 << 31) - 2) * 2048, 8])]          # 2^31 - 1 super-tiles: the largest total that fits (not walked)


def _expected(u, ns):
    counts = [-(-(-(-(n // 8) // 256)) // u) for n in ns]
    first = [sum(counts[:r]) for r in range(len(ns) + 1)]
    return counts, first


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("het_shapes") / "het_shapes_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "dpm_solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "het_shapes_driver.cpp"), "-o", exe], check=True)

    def run(cases):
        text = "".join("%d %d %s\n" % (u, len(ns), " ".join(map(str, ns))) for u, ns in cases)
        out = subprocess.run([exe], input=text, check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [dict(kv.split("=", 1) for kv in line.split()) for line in out]
    return run


def test_the_header_needs_nothing_of_hip():
    src = open(HDR).read()
    incs = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert incs and all(i.startswith("<") and "hip" not in i for i in incs), incs
    assert "__global__" not in src and "threadIdx" not in src and "blockIdx" not in src


def test_the_cases_are_the_ones_asked_for():
    assert {len(ns) for _, ns in CASES} == set(COUNTS) and {u for u, _ in CASES} == {1, 2}
    assert {n for _, ns in CASES for n in ns} == set(SIZES)
    assert all(len(set(ns)) > 1 for _, ns in CASES)


@pytest.fixture(scope="module")
def answers(driver):
    return driver(CASES)


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "u%d_%dreq_%d" % (CASES[i][0], len(CASES[i][1]), i))
def test_plan_lookup_and_grid_walk(answers, i):
    (u, ns), got = CASES[i], answers[i]
    counts, first = _expected(u, ns)
    total = first[-1]
    assert got["fits"] == "1" and got["mixed"] == "1" and int(got["total"]) == total
    # the prefix, padded with the total up to HET_MAX entries
    assert [int(v) for v in got["first"].split(",")] == first + [total] * (HET_MAX - len(ns))
    # v = 0 .. total - 1 visits every (request, local super-tile) exactly once, request-major, and nothing else
    walk = [tuple(map(int, p.split(":"))) for p in got["walk"].split(",")]
    assert walk == [(r, t) for r, c in enumerate(counts) for t in range(c)]
    # every workgroup and 256-lane group of the grid, at 256 and 512 threads, plain and XCD-remapped
    grids = {g.split(":")[0]: g.split(":")[1:] for g in got["grid"].split(",")}
    assert sorted(grids) == ["10", "11", "20", "21"]
    for key, (blocks, ok) in grids.items():
        per, remap = int(key[0]), key[1] == "1"
        span = -(-total // 8)
        assert int(blocks) == (8 * -(-span // per) if remap else -(-total // per)), key
        assert ok == "1", (key, "a super-tile was missed, visited twice or lies outside the plan")


def test_uniform_groups_are_not_mixed_and_bad_groups_have_no_plan(driver):
    for (u, ns), got in zip(UNIFORM, driver(UNIFORM)):
        assert got["fits"] == "1" and got["mixed"] == "0" and int(got["total"]) == _expected(u, ns)[1][-1]
    for got in driver(UNFIT):
        assert got["fits"] == "0" and got["walk"] == "-" and set(got["first"].split(",")) == {"0"}


def test_the_31_bit_limit_is_exact(driver):
    """a total of 2^31 - 1 super-tiles has a plan, 2^31 has none (the launcher then launches the members one by one)"""
    fits, over = driver(ALMOST + [(1, [(1 << 28) * 2048] * 8)])
    assert fits["fits"] == "1" and int(fits["total"]) == (1 << 31) - 1 == _expected(*ALMOST[0])[1][-1]
    assert [int(v) for v in fits["first"].split(",")][:3] == [0, (1 << 31) - 2, (1 << 31) - 1]
    assert over["fits"] == "0" and _expected(1, [(1 << 28) * 2048] * 8)[1][-1] == 1 << 31
