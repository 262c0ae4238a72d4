"""Guard-banded sweep of the launch routes only LARGE sizes reach (tests/guarded.py, the case builders of test_gpu_edges.py).

The launch layer changes a launch's shape -- and in one case the kernel instantiation -- once the launch is large: 512-thread
workgroups from W tiles, a capped grid whose groups loop past K iterations, the cache-resident hot kernels at two tiles per
iteration from W tiles, the one-element-per-lane kernels' grid-stride loop past S elements, the fused shape for a lone launch
from B tiles, the loops of add_noise / blend past A workgroups, a thresholding cluster that walks several samples.  None of
these gates opens below about a million elements, and test_gpu_edges.py stops at 8200.  Here every route runs between guards,
against the numpy doubles bit for bit, at sizes just below, at and past its gate: whole tiles, ragged tails, odd tile counts,
one element past the 16-byte boundary, with the KExt extensions, under classifier guidance, for all five dtype pairs.

The gates W, K, S, B, A are not restated: grid_plan.gates(n_cu) finds them on the answers of tests/grid_plan_driver.cpp, the
host build of csrc/dpm_grid_plan.hpp the launch layer itself calls, at the device's CU count.  `table(n_cu, pair)` is every
cell of the sweep; tests/test_large_routes_host.py runs its doubles and asserts the coverage rule at 256 CUs without a GPU.

Departures from a literal reading of the plan this file was written to, each adding cells, none dropping one:
  * the split mask layout needs n to be a multiple of the tile: the kext variant with it runs at (K+1) T and (2K+5) T, next
    to the looping sizes K T + 8 and (2K+5) T + 16 of the other six;
  * (W+1) T + 8 has an EVEN tile count (the 8 elements open tile W + 2): W T + 8 is added to the resident sizes as the odd one,
    whose last pair has an empty second tile;
  * a thresholding launch of 8 .. 768 elements per sample is one workgroup per sample at any batch (its grid is never capped);
    only clustered samples (more than 12288 elements) share clusters: such a launch with more samples than co-resident clusters
    is added.
Run on an MI355X:  pytest -m gpu tests/test_gpu_large_routes.py
"""
import collections
import ctypes as C
import gc
import re

import numpy as np
import pytest
import torch

import grid_plan as GP
import guarded as G
import kernel_double as KD
import sde_double as SD
import test_gpu_edges as E
from dpm_solver_amd import _lib as L

gpu = pytest.mark.gpu
DEV, T, PAIRS, PAIR_IDS, V = E.DEV, G.T, E.PAIRS, E.PAIR_IDS, E.V
HOST_CU = 256                                   # the CU count test_large_routes_host.py builds the table at
E_PAIRS = [3, 4, 1]                             # fp16/fp16, bf16/bf16, fp32/fp16: the pairs of the big_tiles edge
AUX_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
Cell = collections.namedtuple("Cell", "sec tag n offset family v resident")

HOT = [V(f, store_m=s) for f in ("LIN1", "TWO") for s in (True, False)]          # the cache-resident hot kernels' variants
# the one-element-per-lane route: every form, classifier guidance, a separate evaluation state, eps_stride with batch 2, UniPC
# with STORE_XC, SDE
SCALAR = [("stream", V("LIN1")), ("stream", V("TWO", store_m=False)), ("stream", V("MS3", "classifier-free", "v")),
          ("stream", V("SS3T", sep_xe=True)), ("stream", V("DENOISE", store_m=False)), ("stream", V("TWO", "classifier", "v")),
          ("stream", V("TWO", sep_xe=True)), ("kext", V("LIN1", stride_batch=2, store_m=False)),
          ("unipc", V("UNIPC", dp=True, p2=True, xc=True, dup=True, store_m=False)), ("sde", V("TWO", noise=True))]
RAGGED_BLEND = ("kext", V("MS3", blend="ragged", model="v"))
EDGE = [("TWO", V("TWO")), ("MS3cfg", V("MS3", "classifier-free", dup=True, store_m=False)), ("LIN1cg", V("LIN1", "classifier", "v"))]


def sizes(n_cu):
    """the sizes of every section, from the gates of the launch layer at n_cu CUs"""
    g = GP.gates(n_cu)
    W, K, S, B, A = (g[k] for k in "WKSBA")
    return dict(
        a=[("W-1", (W - 1) * T), ("W", W * T), ("W+g", W * T + 8), ("K", K * T), ("K+g", K * T + 8),
           ("K+1r", (K + 1) * T + 2040 + 3), ("2K+5", (2 * K + 5) * T + 16)],
        a_split=[("K+1", (K + 1) * T), ("2K+5w", (2 * K + 5) * T)],
        b=[("W", W * T), ("W+g", W * T + 8), ("W+1", (W + 1) * T + 8), ("W+1r", W * T + T + 8 * 255 + 5), ("2W", 2 * W * T),
           ("2K", 2 * K * T), ("2K+1", (2 * K + 1) * T + 8), ("2K+3r", (2 * K + 3) * T + 8 * 255 + 5)],
        c=[("S", S, 1), ("S+1", S + 1, 1), ("2S+257", 2 * S + 257, 1), ("S+3", S + 3, 0)],
        e=[("B-1", (B - 1) * T), ("B-1+g", (B - 1) * T + 8), ("B+5", B * T + 5)],
        f_vec=[8 * A * 256, 8 * A * 256 + 8, 16 * A * 256 + 8 * 257],
        f_scalar=[A * 256 + 1, 2 * A * 256 + 257],
        f_blend=[A * 256, A * 256 + 1, 2 * A * 256 + 257],
        g_batch=[2 * n_cu + 1, 4 * n_cu + 3], g_per=[8, 257, 768], g_clustered=(n_cu + 1, 12288 + 8))


def _stream_variant(i, p):
    """variant i of pair p's walk through VARIANTS["stream"] (form-major, twelve (guidance, prologue, STORE_M) combinations per
    form): steps of 13 change the form every time and go through the twelve combinations once per twelve steps"""
    vs = E.VARIANTS["stream"]
    assert len(vs) == 60
    return vs[(13 * i + 7 * p) % 60]


def table(n_cu, p):
    """every cell of the single-request stage sweep (sections a, b, c) of dtype pair p at n_cu CUs"""
    sz, out = sizes(n_cu), []
    for i, (tag, n) in enumerate(sz["a"]):                                         # a: three stream variants per size
        out += [Cell("a", tag, n, 0, "stream", _stream_variant(3 * i + j, p), False) for j in range(3)]
    kext = E.VARIANTS["kext"]
    for (tag, n), (stag, sn) in zip([sz["a"][4], sz["a"][6]], sz["a_split"]):      # a: the seven kext variants, looping sizes
        for v in kext:
            split = v.get("blend") == "split"
            out.append(Cell("a", stag if split else tag, sn if split else n, 0, "kext", v, False))
    for family in ("unipc", "sde"):                                                # a: every unipc / sde variant, looping sizes
        vs = E.VARIANTS[family]
        for i, v in enumerate(vs):
            tag, n = (sz["a"][4], sz["a"][6])[(i + p) % 2]
            out.append(Cell("a", tag, n, 0, family, v, False))
    for i, n in enumerate(E.SIZES):                                                # b: resident at the small sizes
        out.append(Cell("b", "small", n, 0, "stream", HOT[(i + p) % 4], True))
    for i, (tag, n) in enumerate(sz["b"]):                                         # b: two hot variants per large size
        out += [Cell("b", tag, n, 0, "stream", HOT[(2 * i + j + p) % 4], True) for j in range(2)]
    for tag, n, offset in sz["c"]:                                                 # c: the one-element-per-lane route
        for family, v in (SCALAR if offset else [RAGGED_BLEND]):
            out.append(Cell("c", tag, n, offset, family, v, False))
    return out


def edge_table(n_cu):
    """section e: (size tag, n, variant tag, variant, pair index)"""
    return [(tag, n, vt, v, p) for tag, n in sizes(n_cu)["e"] for vt, v in EDGE for p in E_PAIRS]


def n_of(cell):
    return E._n_of(cell.v, cell.n)


def make(cell, p, seed_extra=0):
    sd, ed = PAIRS[p]
    case = E.make_case(cell.family, cell.v, cell.n, sd, ed, cell.offset, seed=cell.n % 100003 + 7 * cell.offset + seed_extra)
    if cell.resident:
        case.resident = True
        case.b = case.buffers()
    return case


def expected_route(cell, p, n_cu):
    """what the launch layer does with the cell, from the driver's answers and the cell's own properties -- the route names the
    coverage rule and the kernel-name checks use: ("vector" | "scalar" | "fused", threads, trips, u)"""
    sd, ed = PAIRS[p]
    v, n = cell.v, n_of(cell)
    blend = E._blend_of(v, n) if v.get("blend") else None
    vec = cell.offset == 0 and not (blend and blend[0] % 8) and not (v.get("stride_batch") and cell.n % 8)
    ext = bool(v.get("dup") or v.get("stride_batch") or blend)
    form, cls, xe = v["form"], v["guidance"] == "classifier", bool(v.get("sep_xe"))
    if v.get("noise") or form == "UNIPC":
        vec = vec and not cls and not xe and (form == "UNIPC" or n % 8 == 0)
    else:
        built = ((not xe and not (form == "DENOISE" and cls)) or form in ("TWO", "SS3T") or (form == "LIN1" and not cls)) \
            and not (form == "SS3T" and (cls or not xe))
        vec = vec and built and not (ext and form == "DENOISE")
    if not vec:
        r = GP.route(n, n_cu)
        return ("scalar", 256, r["scalar_trips"], 1)
    u = 2 if (cell.resident and v in HOT and GP.route(n, n_cu)["big"]) else 1
    r = GP.route(n, n_cu, u)
    return ("vector", r["threads"], r["trips"], u)


# ------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------
def device_cu():
    n, lds = C.c_int(0), C.c_int(0)
    L.check(L.lib.dpm_device_info(C.byref(n), C.byref(lds), C.create_string_buffer(64), 64))
    return n.value


def stage_kernels(fn):
    import test_gpu_unipc_pool as UP
    return UP._stage_kernels(fn)


def template_args(name):
    """the template arguments of a stage kernel's demangled name, casts stripped: stage_kernel<float, __half, 1, 0, false, ...>"""
    m = re.search(r"stage_kernel\w*<(.*)>", name)
    assert m, name
    return [re.sub(r"^\(\w+\)", "", a.strip()) for a in m.group(1).split(",")]


def free():
    gc.collect()
    torch.cuda.empty_cache()


def pure_noise_case(n, sd, offset=0, seed=1000, index=E.NOISE_INDEX, req=0):
    c = G.GuardedLaunch("sde-z", E.noise_stage(index), n, sd, sd, offset=offset, seed=n % 1009, req=req, noise_seed=seed)
    return c


@pytest.fixture(scope="module")
def big_z():
    """section d.  The SDE doubles take the kernel's z; a lone launch of the sizes swept here LOOPS, so its own z would be
    circular.  z of (seed, stage index) comes from a pure-noise two-request dpm_stage_launch_multi -- stage_kernel_multi_noise
    has no loop: one super-tile per 256-lane group -- of the largest size the sweep needs, cached; every n reads a prefix."""
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    n_cu = device_cu()
    sz = sizes(n_cu)
    nz = (max(sz["a"][6][1], 2 * sz["c"][2][1]) + 7) // 8 * 8
    cache, old = {}, SD.Z_SOURCE[0]

    def z(seed, index, n):
        if (seed, index) not in cache:
            devs = [pure_noise_case(nz, torch.float32, seed=seed, index=index, req=r).on(DEV) for r in range(2)]
            arr = (L.Buffers * 2)(*[d.b for d in devs])
            names = stage_kernels(lambda: L.check(L.lib.dpm_stage_launch_multi(C.byref(devs[0].st), arr, 2, E._stream())))
            assert len(names) == 1 and "stage_kernel_multi_noise" in names[0], names
            G.verify_all(devs)
            got = [d.arenas["x_out"].payload().numpy() for d in devs]
            assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32))       # z does not depend on the request
            cache[(seed, index)] = got[0]
            del devs
            free()
        assert n <= nz
        return cache[(seed, index)][:n]
    SD.Z_SOURCE[0] = z
    yield z
    SD.Z_SOURCE[0] = old
    torch.cuda.synchronize()


def run_cell(cell, p, names=None, nonresident_too=False):
    """the double once; the launch on pristine guarded arenas; verify().  names: a list the launch's kernel names are added to"""
    case = make(cell, p)
    want = G.run_double(case)
    for resident in ([cell.resident, False] if nonresident_too else [cell.resident]):
        dev = case.on(DEV)
        if not resident and cell.resident:
            dev.resident = False
            dev.b = dev.buffers()
        assert bool(dev.b.inputs_resident) == resident
        rc = []
        got = stage_kernels(lambda: rc.append(L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), E._stream())))
        torch.cuda.synchronize()
        assert rc == [0], (rc, L.lib.dpm_last_error())
        dev.verify(want)
        if names is not None and resident == cell.resident:
            names += got
        del dev
    del case, want


def _ids(cells):
    return ["%s-%s" % (c[0], c[1]) for c in cells]


# ------------------------------------------------------------------------------------------------
# a, b, c: the single-request stage launch
# ------------------------------------------------------------------------------------------------
A_TAGS = [t for t, _ in sizes(HOST_CU)["a"]]
B_TAGS = ["small"] + [t for t, _ in sizes(HOST_CU)["b"]]
C_TAGS = [t for t, _, _ in sizes(HOST_CU)["c"]]


def _cells(sec, tag, p, n_cu):
    """the cells of one test: a size of a section (the split-layout kext cells ride with the size they stand in for)"""
    alias = dict(zip([t for t, _ in sizes(n_cu)["a_split"]], ("K+g", "2K+5")))
    return [c for c in table(n_cu, p) if c.sec == sec and alias.get(c.tag, c.tag) == tag]


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
@pytest.mark.parametrize("tag", A_TAGS)
def test_streaming_from_hbm(tag, p, big_z):
    """a. U = 1: 256- and 512-thread workgroups, the grid at its cap, a second and a third trip of the loop"""
    n_cu = device_cu()
    for cell in _cells("a", tag, p, n_cu):
        names = []
        run_cell(cell, p, names)
        kind, threads, trips, u = expected_route(cell, p, n_cu)
        print("a %s %s n=%d %s/%s -> %s threads=%d trips=%d: %s" % (tag, PAIR_IDS[p], n_of(cell), cell.family, cell.v["form"], kind,
                                                                   threads, trips, names))
        assert len(names) == 1 and ("_scalar" in names[0]) == (kind == "scalar"), (names, kind)
        if kind == "vector" and cell.family in ("stream", "kext", "unipc"):
            assert template_args(names[0])[6] == "1", names                          # one tile per iteration
    free()


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
@pytest.mark.parametrize("tag", B_TAGS)
def test_resident_hot_kernels(tag, p):
    """b. dpm_buffers.inputs_resident: stage_kernel<..., U, NT = 0> with U = 2 from W tiles and U = 1 below -- the kernel's
    name says which ran --, and the same buffers without the field give the same bits (both are held to the same double)"""
    n_cu = device_cu()
    for cell in _cells("b", tag, p, n_cu):
        names = []
        run_cell(cell, p, names, nonresident_too=True)
        kind, threads, trips, u = expected_route(cell, p, n_cu)
        print("b %s %s n=%d %s -> U=%d threads=%d trips=%d: %s" % (tag, PAIR_IDS[p], cell.n, cell.v["form"], u, threads, trips, names))
        assert kind == "vector" and len(names) == 1 and "stage_kernel<" in names[0], names
        args = template_args(names[0])
        assert args[6:8] == [str(u), "0"], (names, u)                               # U, NT
        assert u == (2 if tag != "small" else 1)
    free()


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
@pytest.mark.parametrize("tag", C_TAGS)
def test_one_element_per_lane(tag, p, big_z):
    """c. stage_kernel_scalar, _scalar_unipc, _scalar_noise at and past their grid cap"""
    n_cu = device_cu()
    for cell in _cells("c", tag, p, n_cu):
        names = []
        run_cell(cell, p, names)
        kind, threads, trips, u = expected_route(cell, p, n_cu)
        print("c %s %s n=%d %s/%s trips=%d: %s" % (tag, PAIR_IDS[p], n_of(cell), cell.family, cell.v["form"], trips, names))
        want = {"unipc": "stage_kernel_scalar_unipc", "sde": "stage_kernel_scalar_noise"}.get(cell.family, "stage_kernel_scalar<")
        assert kind == "scalar" and len(names) == 1 and want in names[0], names
    free()


# ------------------------------------------------------------------------------------------------
# d: the z the SDE doubles take
# ------------------------------------------------------------------------------------------------
@gpu
def test_looping_launches_draw_the_contracts_z(big_z):
    """the lone LOOPING launch's pure-noise output -- vector route at K T + 8 and (2K+5) T + 16, one-element-per-lane route at
    2S + 257 (offset 1) and S + 3 -- equals the loop-free fused launch's z bit for bit, and that z sits within the bound
    test_gpu_edges.py::test_sde_noise_contract applies to the float64 restatement"""
    n_cu = device_cu()
    sz = sizes(n_cu)
    seed, index = 0x0123456789ABCDEF, 5
    cells = [(sz["a"][4][1], 0, "vector"), (sz["a"][6][1], 0, "vector"), (sz["c"][2][1], 1, "scalar"), (sz["c"][3][1], 0, "scalar")]
    nmax = max(n for n, _, _ in cells)
    z = big_z(seed, index, nmax).astype(np.float64)
    want = SD.noise_z64(seed, index, nmax)
    assert np.all(np.abs(z - want) <= 1e-5 * np.maximum(1.0, np.abs(want))), float(np.max(np.abs(z - want)))
    del z, want
    for n, offset, kind in cells:
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            case = pure_noise_case(n, dt, offset, seed=seed, index=index)
            wanted = G.run_double(case)
            dev = case.on(DEV)
            names = stage_kernels(lambda: L.check(L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), E._stream())))
            dev.verify(wanted)
            r = GP.route(n, n_cu)
            assert len(names) == 1 and ("stage_kernel_scalar_noise" in names[0]) == (kind == "scalar"), names
            assert (r["scalar_trips"] if kind == "scalar" else r["trips"]) >= 2, (n, r)
            del dev, case, wanted
        free()


# ------------------------------------------------------------------------------------------------
# e: the big_tiles edge
# ------------------------------------------------------------------------------------------------
def edge_case(n, v, p):
    sd, ed = PAIRS[p]
    return E.make_case("stream", v, n, sd, ed, 0, seed=n % 100003)


def edge_fused(n, v, n_cu):
    """does the lone launch come back from the fused family as a launch?  The driver says whether it is offered; the fused
    family declines classifier guidance and ragged sizes (fusable_request)"""
    return bool(GP.route(n, n_cu)["fused"]) and v["guidance"] != "classifier" and n % 8 == 0


@gpu
@pytest.mark.parametrize("tag,n,vt,v,p", edge_table(HOST_CU), ids=["%s-%s-%s" % (t, vt, PAIR_IDS[p]) for t, _, vt, _, p in edge_table(HOST_CU)])
def test_big_tiles_edge(tag, n, vt, v, p):
    """e. one tile below big_tiles the capped loop runs its longest; at big_tiles the launch is the fused kernel's group of one;
    what that family declines comes back and loops"""
    n_cu = device_cu()
    n = dict(sizes(n_cu)["e"])[tag]
    want = G.run_double(edge_case(n, v, p))
    dev = want.on(DEV)
    rc = []
    names = stage_kernels(lambda: rc.append(L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), E._stream())))
    torch.cuda.synchronize()
    assert rc == [0], (rc, L.lib.dpm_last_error())
    dev.verify(want)
    print("e %s %s %s n=%d: %s" % (tag, vt, PAIR_IDS[p], n, names))
    assert len(names) == 1 and ("stage_kernel_multi" in names[0]) == edge_fused(n, v, n_cu), names
    del dev, want
    free()


# ------------------------------------------------------------------------------------------------
# f: dpm_add_noise_launch, dpm_blend_launch
# ------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(G._INT[t.element_size()])


def add_noise_cells(n_cu):
    return [("vec", i, nt, 0) for i in range(3) for nt in (1, 3)] + [("scalar", i, nt, (0, 1)[nt == 3]) for i in range(2) for nt in (1, 3)]


def add_noise_operands(n, nt, dt):
    g = torch.Generator().manual_seed(n % 100003 + nt)
    return (torch.randn(n, generator=g) * 1.7).to(dt), torch.randn(nt, n, generator=g).to(dt), np.array([0.3, 0.9, 0.05][:nt], dtype=np.float32)


def schedule():
    import dpm_solver_amd as D
    return D.NoiseScheduleVP("discrete", betas=torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64))


@gpu
@pytest.mark.parametrize("dt", AUX_DTYPES, ids=[G._name(d) for d in AUX_DTYPES])
@pytest.mark.parametrize("route,i,nt,offset", add_noise_cells(HOST_CU), ids=["%s%d-nt%d" % c[:3] for c in add_noise_cells(HOST_CU)])
def test_add_noise_past_the_grid_cap(route, i, nt, offset, dt):
    """f. add_noise_kernel<T, true> (8 elements per lane) and <T, false> (ragged n, or one element past the 16-byte boundary)
    with their grid-stride loops taken, against kernel_double.add_noise_double, the output between guards"""
    n_cu = device_cu()
    n = sizes(n_cu)["f_vec" if route == "vec" else "f_scalar"][i]
    r = GP.route(n, n_cu)
    assert (n % 8 == 0 and offset == 0) == (route == "vec")
    ns = schedule()
    xs, nz, th = add_noise_operands(n, nt, dt)
    want = KD.add_noise_double(ns._h, xs, nz, th)
    x, noise = G.Arena(dt, n, DEV, offset, bits=_bits(xs)), G.Arena(dt, nt * n, DEV, offset, bits=_bits(nz).reshape(-1))
    out = G.Arena(dt, nt * n, DEV, offset)
    rc = L.lib.dpm_add_noise_launch(ns._h, th.ctypes.data_as(C.POINTER(C.c_float)), nt, x.ptr, noise.ptr, out.ptr, n, G.CODE[dt],
                                    E._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    x.verify("x"), noise.verify("noise")
    out.verify("add_noise %s n=%d nt=%d trips=%d" % (route, n, nt, r["aux_vec_trips" if route == "vec" else "aux_trips"]),
               _bits(want.to(dt)).reshape(-1))
    del x, noise, out
    free()


def blend_double(xs, mk, av, bv, alpha, sigma, dt):
    """kernel_double.blend with the mask indexed i % period, as dpm_blend_launch reads it"""
    m = KD._np(mk)[np.arange(xs.numel()) % mk.numel()]
    res = KD.blend(alpha, sigma, KD._np(xs), m, KD._np(av), None if bv is None else KD._np(bv))
    return torch.from_numpy(np.ascontiguousarray(res)).to(dt)


@gpu
@pytest.mark.parametrize("dt", AUX_DTYPES, ids=[G._name(d) for d in AUX_DTYPES])
@pytest.mark.parametrize("i", range(3))
def test_blend_past_the_grid_cap(i, dt):
    """f. blend_kernel at, one element past and twice past its grid cap: mask periods n, 64 and 7, with and without blend_b"""
    n_cu = device_cu()
    n = sizes(n_cu)["f_blend"][i]
    alpha, sigma = float(np.float32(0.8)), float(np.float32(0.6))
    g = torch.Generator().manual_seed(n % 100003)
    xs, av, bv = (torch.randn(n, generator=g).to(dt) for _ in range(3))
    for period in (n, 64, 7):
        mk = torch.rand(period, generator=g).to(dt)
        for with_b in (True, False):
            want = blend_double(xs, mk, av, bv if with_b else None, alpha, sigma, dt)
            ar = {k: G.Arena(dt, t.numel(), DEV, bits=_bits(t)) for k, t in (("x", xs), ("mask", mk), ("a", av), ("b", bv))}
            out = G.Arena(dt, n, DEV)
            rc = L.lib.dpm_blend_launch(ar["x"].ptr, ar["mask"].ptr, ar["a"].ptr, ar["b"].ptr if with_b else None, alpha, sigma,
                                        out.ptr, n, period, G.CODE[dt], E._stream())
            torch.cuda.synchronize()
            assert rc == 0, (rc, L.lib.dpm_last_error())
            for k, a in ar.items():
                a.verify(k)
            out.verify("blend n=%d period=%d blend_b=%s trips=%d" % (n, period, with_b, GP.route(n, n_cu)["aux_trips"]), _bits(want))
            del ar, out
    free()


# ------------------------------------------------------------------------------------------------
# g: thresholding with more samples than resident workgroups
# ------------------------------------------------------------------------------------------------
def thresh_cells(n_cu):
    sz = sizes(n_cu)
    out = [(b, per) for b in sz["g_batch"] for per in sz["g_per"]]
    return out + [sz["g_clustered"]]


def run_thresh(cases):
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    arr = (L.Buffers * len(cases))(*[d.b for d in devs])
    if len(cases) == 1:
        rc = L.lib.dpm_stage_launch(C.byref(devs[0].st), arr, E._stream())
    else:
        rc = L.lib.dpm_stage_launch_multi(C.byref(devs[0].st), arr, len(cases), E._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants, rc)


@gpu
@pytest.mark.parametrize("p", [0, 3], ids=[PAIR_IDS[0], PAIR_IDS[3]])
@pytest.mark.parametrize("i", range(len(thresh_cells(HOST_CU))))
def test_thresholding_more_samples_than_workgroups(i, p):
    """g. batches of 2C + 1 and 4C + 3 samples of 8, 257 and 768 elements (one workgroup per sample: the grid is the batch), and
    C + 1 samples of 12296 elements: two workgroups per sample, at most C clusters co-resident -- a cluster walks two samples"""
    n_cu = device_cu()
    batch, per = thresh_cells(n_cu)[i]
    sd, ed = PAIRS[p]
    clustered = int(L.lib.dpm_threshold_workspace_bytes(batch, per)) > 0
    assert clustered == (per > 12288)
    variants = [("TWO", "uncond"), ("MS3", "classifier-free")]
    for form, guidance in (variants[p % 2:][:1] if clustered else variants):
        run_thresh([E.thresh_case(form, guidance, per, batch, sd, ed, seed=per + batch)])
    free()


@gpu
def test_thresholding_three_requests_of_many_samples():
    """g. one multi-request call of three requests of 2C + 1 samples each"""
    n_cu = device_cu()
    sd, ed = PAIRS[3]
    batch, per = sizes(n_cu)["g_batch"][0], 257
    run_thresh([E.thresh_case("LIN1", "classifier-free", per, batch, sd, ed, req=r, seed=per + batch) for r in range(3)])
    free()
