"""The table-mode call with EVERY row kind in it at once, LAUNCHED, on the MI355X: the GPU counterpart of
tests/test_table_kinds_host.py, whose 29-request KINDS order and runs(flags) expectation it imports.  Kernel level, through the
C ABI and between guards (tests/guarded.py), as tests/test_gpu_table.py and its three siblings -- each of which sets at most two
of the flags: plain / UniPC, MS3, SDE (two model types), thresholded (two ratios), mask-blend and ragged requests interleaved
in call order go DPM_TABLE_FILL | flags into a poisoned host tensor, `copy_` to a guard-banded device table,
DPM_TABLE_LAUNCH | flags.  Every request is compared three ways: with its numpy double (an SDE request's double takes the
kernel's own z), with its own dpm_stage_launch, and with the same arrays in mode 0 -- bit for bit.  The table and its guards must
be as the host wrote them, the header [MAGIC, version, 29, runs], and the launches, by kernel name, one table kernel of the right
family per run, in the runs' order, plus the launches mode 0 gives the requests that own no row.

The flag words: all three flags, each flag cleared in turn, none.  A cleared flag takes its kind's requests out of the table and
must leave them their bits: each flag word is compared with the same double and the same single launches, and the first flag
word a (dtype pair, cell) ran with every later one.  One more variant moves the kinds: a thresholded row owner is request 0 and
the plain group opens last.

Shapes, the smallest at which these kernels differ in path: plain / SDE / blend n of 2056 (a 2048-tile and one 8-group), 8 (one
group), 4104; thresholded samples of 2056 x 2, 8 x 3 and 12288 x 1 (the largest a row holds).
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import pytest
import torch

import guarded as G
import sde_double as SD
import test_gpu_edges as E
from dpm_solver_amd import _lib as L
from test_gpu_edges import PAIRS, PAIR_IDS
from test_gpu_pool_shapes import requests
from test_gpu_table import DEV, TableCall, _stream
from test_gpu_table_blend import blend_requests
from test_gpu_table_thresh import thr_requests
from test_table_kinds_host import ALL, KINDS, runs

gpu = pytest.mark.gpu
# (cell, n of a plain / SDE / blend request, elements per thresholded sample, samples per thresholded request)
CELLS = [("a", 2056, 2056, 2), ("b", 8, 8, 3), ("c", 4104, 12288, 1)]
FLAG_WORDS = [ALL, ALL & ~L.TABLE_NOISE, ALL & ~L.TABLE_THRESH, ALL & ~L.TABLE_BLEND, 0]
FLAG_IDS = ["all", "no-noise", "no-thresh", "no-blend", "none"]
COMBOS = [(g, m) for g in ("uncond", "classifier-free") for m in ("noise", "v")]      # guidance x prologue (v: generic)
# the kinds moved: a thresholded row owner is request 0, every other group opens before the plain one
MOVED = (["thr", "sde", "blend", "sde_v", "thr_b", "ragged", "sde", "thr", "blend", "plain", "plain", "unipc", "ms3", "plain", "unipc"]
         + ["plain"] * 14)
TABLE_MIN = 17                                    # members from which a plain / UniPC group owns rows
# the group a kind of request joins, the flag its rows need, the kind of its run, the kernel family of its run
GROUP = {"plain": "plain", "unipc": "plain", "sde": "sde", "sde_v": "sde_v", "thr": "thr", "thr_b": "thr_b", "blend": "blend"}
NEEDS = {"plain": 0, "sde": L.TABLE_NOISE, "sde_v": L.TABLE_NOISE, "thr": L.TABLE_THRESH, "thr_b": L.TABLE_THRESH, "blend": L.TABLE_BLEND}
RUN_KIND = {"plain": "plain", "sde": "sde", "sde_v": "sde", "thr": "thr", "thr_b": "thr", "blend": "blend"}
FAMILY = {"thr": "stage_thresh_kernel_table", "sde": "stage_kernel_table_noise", "blend": "stage_kernel_table_blend",
          "plain": "stage_kernel_table_unipc"}    # (the plain group holds UniPC records: that family's table kernel)


def combo_of(p, ci):
    return COMBOS[(p + ci) % len(COMBOS)]


def runs_of(kinds, flags):
    """runs(flags) of tests/test_table_kinds_host.py for any order of kinds: the groups in the order they open, members in call
    order; a group owns a run if the call carries its flag and it has its kind's least number of members"""
    groups = {}
    for r, k in enumerate(kinds):
        g = GROUP.get(k)                          # (MS3 behind a UniPC record, and the ragged request: no group)
        if g is not None and not NEEDS[g] & ~flags:
            groups.setdefault(g, []).append(r)
    return [(RUN_KIND[g], members) for g, members in groups.items() if len(members) >= (TABLE_MIN if g == "plain" else 1)]


def lone_launches(kinds, flags):
    """the launches of the requests that own no row, as mode 0 gives them: (fused launches of two or more members -- SDE
    requests of one model type whose flag is cleared --, launches of one request)"""
    rowed = {r for _, members in runs_of(kinds, flags) for r in members}
    rest = [kinds[r] for r in range(len(kinds)) if r not in rowed]
    assert "plain" not in rest and "unipc" not in rest       # (so the MS3 request finds nobody to share a launch with)
    fused = [k for k in ("sde", "sde_v") if rest.count(k) >= 2]
    return len(fused), len([k for k in rest if k not in fused])


def test_rotation_covers_guidance_prologue_and_flag_words():
    assert len(PAIRS) == 5 and len(FLAG_WORDS) == len(set(FLAG_WORDS)) == 5 and FLAG_WORDS[0] == ALL and FLAG_WORDS[-1] == 0
    for p in range(len(PAIRS)):                   # every dtype pair meets both guidances and both network kinds
        met = [combo_of(p, ci) for ci in range(len(CELLS))]
        assert {g for g, _ in met} == {"uncond", "classifier-free"} and {m for _, m in met} == {"noise", "v"}, p
    # every cell meets every flag word: the parametrisation of the GPU test is the full product
    assert {(ci, f) for ci, f, _ in _cases()} == {(ci, f) for ci in range(len(CELLS)) for f in range(len(FLAG_WORDS))}
    assert {p for _, _, p in _cases()} == set(range(len(PAIRS)))
    # the restated walk is the host test's expectation, for every flag word
    for flags in FLAG_WORDS:
        assert runs_of(KINDS, flags) == runs(flags)
    # the moved kinds: the same multiset, a thresholded request first, the plain group last, MS3 behind a UniPC record
    assert sorted(MOVED) == sorted(KINDS) and MOVED[0] == "thr" and MOVED.index("unipc") < MOVED.index("ms3")
    moved = runs_of(MOVED, ALL)
    assert [k for k, _ in moved] == ["thr", "sde", "blend", "sde", "thr", "plain"] and moved[0][1][0] == 0
    assert sorted(len(m) for _, m in moved) == sorted(len(m) for _, m in runs(ALL))
    assert lone_launches(KINDS, ALL) == (0, 2) and lone_launches(KINDS, 0) == (1, 8)


def _cases():
    return [(ci, f, p) for p in range(len(PAIRS)) for ci in range(len(CELLS)) for f in range(len(FLAG_WORDS))]


def _reseed(case, seed, index):
    """an SDE request with a seed and a stage index of its own"""
    case.kw["noise_seed"], case.st.index = seed, index
    case.opts.noise_seed_lo, case.opts.noise_seed_hi = seed & 0xFFFFFFFF, seed >> 32
    return case


def build(kinds, p, ci):
    """the CPU cases of one call in the order of `kinds`, by the helpers of the sibling files, and their doubles"""
    sd, ed = PAIRS[p]
    _, n, per, batch = CELLS[ci]
    guidance, model = combo_of(p, ci)
    other = "v" if model == "noise" else "noise"
    seed = 7 * p + ci
    count = {k: kinds.count(k) for k in set(kinds)}
    unipc = requests("unipc", guidance, model, 6, sd, ed, seed=seed + 1, sizes=[n] * 6)
    assert unipc[0].st.form == unipc[5].st.form == L.FORM_UNIPC and count["unipc"] == 2
    ms3 = requests("het3", guidance, model, 3, sd, ed, seed=seed + 2, sizes=[n] * 3)[2]
    assert ms3.st.form == L.FORM_MS3
    pools = {
        "plain": requests("het2", guidance, model, count["plain"], sd, ed, seed=seed, sizes=[n] * count["plain"]),
        "unipc": [unipc[0], unipc[5]],
        "ms3": [ms3],
        "sde": [_reseed(c, 0x1000 + r, 1 + r) for r, c in enumerate(
            requests("noise", guidance, model, count["sde"], sd, ed, seed=seed + 3, sizes=[n] * count["sde"]))],
        "sde_v": [_reseed(c, (1 << 63) + 9, 3) for c in requests("noise", guidance, other, 1, sd, ed, seed=seed + 4, sizes=[n])],
        "thr": thr_requests(count["thr"], per, batch, sd, ed, guidance, model, 0.995, (0.25, 100.0)[(p + ci) % 2], seed=seed + 5),
        "thr_b": thr_requests(1, per, batch, sd, ed, guidance, model, 0.5, (0.25, 100.0)[(p + ci) % 2], seed=seed + 6),
        "blend": blend_requests(count["blend"], n, guidance, model, sd, ed, seed=seed + 7),
        "ragged": requests("het2", guidance, model, 1, sd, ed, seed=seed + 8, sizes=[n + 3]),
    }
    assert all(len(pools[k]) == count[k] for k in count) and (n + 3) % 8 != 0
    took = {k: 0 for k in pools}
    cases = []
    for k in kinds:
        cases.append(pools[k][took[k]])
        took[k] += 1
    cache, old = {}, SD.Z_SOURCE[0]

    def z(zseed, index, m):                       # the kernel's own z, as test_plain_sde_and_blend_groups_each_get_their_kernel
        if (zseed, index) not in cache:
            cache[(zseed, index)] = E.kernel_z(zseed, index, n)
        return cache[(zseed, index)][:m]
    SD.Z_SOURCE[0] = z
    try:
        wants = [G.run_double(c) for c in cases]
    finally:
        SD.Z_SOURCE[0] = old
    return cases, wants


_SHARED = {}                                      # the last (kinds, p, ci) built: cases, doubles, the first flag word's output bits


def shared(name, kinds, p, ci):
    if _SHARED.get("key") != (name, p, ci):
        _SHARED.clear()
        cases, wants = build(kinds, p, ci)
        _SHARED.update(key=(name, p, ci), cases=cases, wants=wants, bits=None)
    return _SHARED


def _refill(d):
    for k in G.OUTPUTS:
        d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])


def _outputs(devs):
    return [{k: d.arenas[k].raw.clone() for k in G.OUTPUTS} for d in devs]


def _same(devs, bits, what):
    for r, d in enumerate(devs):
        for k in G.OUTPUTS:
            assert torch.equal(bits[r][k], d.arenas[k].raw), (r, d.n, k, what)


def _family(name):
    for kind in ("thr", "sde", "blend"):
        if FAMILY[kind] in name:
            return kind
    return "plain" if "stage_kernel_table" in name else None


def _launched(fn):
    """the stage kernels fn() launches, in launch order: _names of tests/test_gpu_table_thresh.py (torch's profiler, the first
    call outside the profile) read from the profile's events, which keep the order its per-name averages drop"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    keep = lambda s: "stage_kernel" in s or "stage_thresh_kernel" in s
    names = [e.key for e in sorted(prof.events(), key=lambda e: e.time_range.start) if keep(e.key)]
    assert sorted(names) == sorted(e.key for e in prof.key_averages() if keep(e.key) for _ in range(e.count))
    return names


def check_kinds_call(name, kinds, p, ci, flags):
    sh = shared(name, kinds, p, ci)
    wants, devs = sh["wants"], [c.on(DEV) for c in sh["cases"]]
    want_runs = runs_of(kinds, flags)
    t = TableCall(devs, flags)
    assert t.host.numel() == L.table_bytes(len(kinds), flags)
    # 1. the call, against the doubles
    t.tick()
    G.verify_all(devs, wants)
    assert t.table_intact(), "the kernels may only read their table"
    assert t.host[:16].view(torch.int32).tolist() == [L.TABLE_MAGIC, L.lib.dpm_version(), len(kinds), len(want_runs)]
    fused = _outputs(devs)
    if sh["bits"] is None:
        sh["bits"] = [{k: v.cpu() for k, v in f.items()} for f in fused]
    for r, f in enumerate(fused):                 # a cleared flag leaves its kind's requests their bits
        for k in G.OUTPUTS:
            assert torch.equal(f[k].cpu(), sh["bits"][r][k]), (r, kinds[r], k, "differs from the call under another flag word")
    # 2. every request's own dpm_stage_launch
    for d in devs:
        _refill(d)
        rc = L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
    _same(devs, fused, "differs from the request's own dpm_stage_launch")
    # 3. the same arrays in mode 0
    for d in devs:
        _refill(d)
    t.mode0()
    _same(devs, fused, "differs from the same arrays in mode 0")
    G.verify_all(devs, wants)
    # 4. the launches, by kernel name: one table kernel per run, of the run's family, in the runs' order ...
    for d in devs:
        _refill(d)
    names = _launched(t.tick)
    _same(devs, fused, "differs on the profiled tick")
    assert t.table_intact()
    tables = [_family(k) for k in names if _family(k)]
    assert tables == [kind for kind, _ in want_runs], names
    assert all(FAMILY[kind] in k for kind, k in zip(tables, [k for k in names if _family(k)])), names
    # ... and the requests that own no row as mode 0 launches them
    n_fused, n_lone = lone_launches(kinds, flags)
    assert len(names) == len(want_runs) + n_fused + n_lone, names
    assert sum("stage_kernel_het_noise" in k for k in names) == n_fused, names
    # (a thresholded request without DPM_TABLE_THRESH: its own clustered launch)
    thr_lone = 0 if flags & L.TABLE_THRESH else kinds.count("thr") + kinds.count("thr_b")
    assert sum("stage_thresh_kernel" in k and _family(k) is None for k in names) == thr_lone, names


@gpu
@pytest.mark.parametrize("f", range(len(FLAG_WORDS)), ids=FLAG_IDS)
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=[c[0] for c in CELLS])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_every_kind_in_one_launched_call(p, ci, f):
    assert KINDS[0] == "plain"                    # (request 0 plain: bs[0].workspace is free for the table)
    assert runs_of(KINDS, FLAG_WORDS[f]) == runs(FLAG_WORDS[f])      # every count below comes from the host test's expectation
    check_kinds_call("kinds", KINDS, p, ci, FLAG_WORDS[f])


@gpu
@pytest.mark.parametrize("ci", range(len(CELLS)), ids=[c[0] for c in CELLS])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_the_kinds_moved_a_thresholded_row_first_the_plain_group_last(p, ci):
    """no check depends on plain rows coming first: request 0 owns a thresholded row (the call's bs[0].workspace is the table,
    its own launch and the mode-0 call get the workspace its cluster needs), the 19 plain / UniPC rows are the last run"""
    check_kinds_call("moved", MOVED, p, ci, ALL)
