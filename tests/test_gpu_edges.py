"""Guard-banded tile-edge sweep of every stage-kernel family through the C ABI (tests/guarded.py): each launch runs on
operands that sit between 8192-element guards, at sizes derived from the kernels' constants (8 elements per lane group, 2048
per tile) -- one group, one group short of a tile, odd tile counts, multi-tile sizes with a ragged tail -- and at request
counts that put a fused launch's super-tile total below, at and around the 8-way XCD span and across HET_MAX = 16 and
DPM_MULTI_MAX = 32.  `verify()` checks the guards, the inputs, the outputs a stage must not write, that no payload element was
skipped, and the bits against the numpy doubles.  Which (size, request count, offset) cells every family x dtype pair runs is
a table (`cells`, `plan`); test_table_meets_the_coverage_rule asserts the rule on it.  Run on an MI355X:  pytest -m gpu
"""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import guarded as G
import sde_double as SD
from dpm_solver_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
T = G.T
WHOLE = [8, T - 8, T, T + 8, 2 * T - 8, 2 * T, 2 * T + 8, 3 * T, 3 * T + 8, 4 * T + 8]
RAGGED = [1, 7, 9, T - 1, T + 1, 2 * T + 7, 3 * T + 9]
SIZES = WHOLE + RAGGED
COUNTS = [1, 2, 3, 7, 8, 9, 16, 17, 32, 33]
OFFSET1 = [T + 8, 3 * T, 2 * T + 7]                       # the sizes that also run one element past the 16-byte boundary
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
         (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)]
PAIR_IDS = ["%s-%s" % (G._name(s), G._name(e)) for s, e in PAIRS]
THR_SIZES = [8, 9, 255, 256, 257, T, T + 1, 3 * 16 * 16]      # one workgroup per sample: no workspace (0 bytes)
THR_CLUSTERED = [2 * T, 2 * T + 9]                            # two workgroups per sample: they exchange through the workspace
THR_BATCHES = (1, 3)
NOISE_INDEX, NZ = 3, 4 * T + 16                           # stage index of every SDE stage here; elements of the reference z


# ------------------------------------------------------------------------------------------------
# the table: variants per family, cells per kind of family
# ------------------------------------------------------------------------------------------------
def V(form, guidance="uncond", model="noise", store_m=True, **kw):
    return dict(form=form, guidance=guidance, model=model, store_m=store_m, **kw)


_F = {"LIN1": L.FORM_LIN1, "TWO": L.FORM_TWO, "MS3": L.FORM_MS3, "SS3T": L.FORM_SS3T, "DENOISE": L.FORM_DENOISE,
      "UNIPC": L.FORM_UNIPC}
UNIPC_SHAPES = [(False, False), (False, True), (True, False), (True, True)]
VARIANTS = {
    # forms x guidance x (compile-time prologue: noise network + TO_X0 | generic prologue: v network) x STORE_M
    "stream": [V(f, g, m, s, sep_xe=(f == "SS3T")) for f in ("LIN1", "TWO", "MS3", "SS3T", "DENOISE")
               for g in ("uncond", "classifier-free", "classifier") for m in ("noise", "v") for s in (True, False)],
    # CFG duplicate store; eps_stride = 2 x per_sample with batch 2 and 3 (the size is the PER-SAMPLE size there: n = batch x
    # size); mask blend with a split-layout period (T, where it divides n), a pack-layout period (8) and a ragged period
    "kext": [V("TWO", "classifier-free", dup=True), V("LIN1", stride_batch=2, store_m=False),
             V("MS3", "classifier-free", stride_batch=3), V("TWO", blend="split", store_m=False),
             V("LIN1", "classifier-free", blend="pack", dup=True), V("MS3", blend="ragged", model="v"),
             V("LIN1", "classifier-free", blend="pack", blend_b=False, dup=True, store_m=False)],
    "unipc": [V("UNIPC", g, m, s, dp=dp, p2=p2, xc=xc, dup=(xc or g != "uncond"))
              for dp, p2 in UNIPC_SHAPES for g, m, xc, s in (("uncond", "noise", False, True), ("uncond", "noise", True, False),
                                                             ("classifier-free", "noise", False, False),
                                                             ("uncond", "v", False, True))],
    "sde": [V(f, g, m, (i + j) % 2 == 0, noise=True, dup=(g != "uncond")) for i, f in enumerate(("LIN1", "TWO"))
            for g in ("uncond", "classifier-free") for j, m in enumerate(("noise", "v"))],
    # the forms of stage_kernel_multi (UNIPC in its four sub-shapes) and of stage_kernel_multi_noise, unguided and
    # classifier-free, noise and v networks (compile-time and generic prologue), with and without STORE_M
    "lockstep": [V(f, g, ("v" if (i + j) % 3 == 2 else "noise"), (i + j) % 2 == 0, dup=(g != "uncond"), dp=dp, p2=p2, noise=nz)
                 for i, (f, nz, dp, p2) in enumerate([("LIN1", False, 0, 0), ("TWO", False, 0, 0), ("MS3", False, 0, 0),
                                                      ("UNIPC", False, False, False), ("UNIPC", False, False, True),
                                                      ("UNIPC", False, True, False), ("UNIPC", False, True, True),
                                                      ("LIN1", True, 0, 0), ("TWO", True, 0, 0)])
                 for j, g in enumerate(("uncond", "classifier-free"))],
    # per-request stages: the forms a call mixes -- stage_kernel_het with two and three forms, _het_noise, _het_unipc
    "het": [V(mix, g, ("v" if (i + j) % 3 == 2 else "noise"), dup=(g != "uncond"))
            for i, mix in enumerate(("het2", "het3", "noise", "unipc")) for j, g in enumerate(("uncond", "classifier-free"))],
    "f64": [V(f, g, sep_xe=(f == "SS3T"), dup=(g == "classifier-free")) for f in ("LIN1", "TWO", "MS3", "SS3T", "DENOISE")
            for g in ("uncond", "classifier-free", "classifier")] + [V("TWO", blend="pack"), V("LIN1", blend="ragged", blend_b=False)],
}
HET_MIX = {"het2": ("LIN1", "TWO"), "het3": ("LIN1", "TWO", "MS3"), "noise": ("LIN1", "TWO"), "unipc": ("LIN1", "UNIPC", "TWO")}
FUSED = ("lockstep", "het")
PER_CELL = {"stream": 3, "kext": 7, "unipc": 2, "sde": 2, "lockstep": 2, "het": 2, "f64": 3}


def cells(family):
    """(n, request count, offset) of every launch of a family, in a fixed order"""
    if family not in FUSED:
        return [(n, 1, 0) for n in SIZES] + [(n, 1, 1) for n in OFFSET1]
    out = [(n, c, 0) for n in SIZES for c in (1, 3, 9)]
    out += [(n, c, 0) for c in COUNTS for n in (8, T + 8, 3 * T) if (n, c, 0) not in out]
    return out + [(n, 3, 1) for n in OFFSET1]


def plan(family, pair_index=0):
    """[(cell, variant)]: every cell with PER_CELL[family] variants in rotation -- all of them at offset 1 for the
    single-launch families (the one-element-per-lane route of every variant).  The variants are shuffled per dtype pair
    (fixed seed), so that a form is not tied to the sizes next to it in the list"""
    vs, k, out = list(VARIANTS[family]), PER_CELL[family], []
    random.Random(97 * pair_index + len(vs)).shuffle(vs)
    for i, cell in enumerate(cells(family)):
        every = cell[2] == 1 and family not in FUSED
        idx = range(len(vs)) if every else [(i * k + j) % len(vs) for j in range(k)]
        out += [(cell, vs[j]) for j in idx]
    return out


def test_table_meets_the_coverage_rule():
    assert len(PAIRS) == 5 and len(set(PAIRS)) == 5 and G.GUARD >= 8192 and G.GUARD >= 2 * 2 * T
    assert WHOLE == [8, 2040, 2048, 2056, 4088, 4096, 4104, 6144, 6152, 8200] and RAGGED == [1, 7, 9, 2047, 2049, 4103, 6153]
    assert THR_SIZES == [8, 9, 255, 256, 257, 2048, 2049, 768]
    for family in VARIANTS:
        for p in range(len(PAIRS)):
            pl = plan(family, p)
            got = {c for c, _ in pl}
            counts = (1, 3, 9) if family in FUSED else (1,)
            assert all((n, c, 0) in got for n in SIZES for c in counts), family
            if family in FUSED:
                assert all((n, c, 0) in got for c in COUNTS for n in (8, T + 8, 3 * T)), family
            assert len({n for n, c, o in got if o == 1}) >= 3 and all((n, c, 0) in got for n, c, o in got if o == 1), family
            used = [v for _, v in pl]
            assert all(v in used for v in VARIANTS[family]), (family, p)                 # no variant a rotation never reaches
            if family == "unipc":                                                          # STORE_XC at offsets 0 and 1
                assert {c[2] for c, v in pl if v.get("xc")} == {0, 1}
            if family == "kext":                                                           # the three mask layouts are met
                kinds = {_blend_of(v, _n_of(v, c[0]))[2] for c, v in pl if v.get("blend")}
                assert kinds == {"split", "pack", "ragged"}
                assert {v["stride_batch"] for _, v in pl if v.get("stride_batch")} == {2, 3}
    forms = {v["form"] for v in VARIANTS["stream"]}
    assert forms == {"LIN1", "TWO", "MS3", "SS3T", "DENOISE"}
    for f in forms:       # every form: unguided / CFG / classifier x compile-time / generic prologue x STORE_M on / off
        assert {(v["guidance"], v["model"], v["store_m"]) for v in VARIANTS["stream"] if v["form"] == f} == {
            (g, m, s_) for g in ("uncond", "classifier-free", "classifier") for m in ("noise", "v") for s_ in (True, False)}, f
    for family in VARIANTS:                                                # m_out untouched without STORE_M: every family
        assert {v["store_m"] for v in VARIANTS[family]} == {True, False} or family in ("het", "f64"), family
    for family in ("lockstep", "het", "unipc", "sde", "kext"):             # compile-time and generic prologue
        assert {v["model"] for v in VARIANTS[family]} == {"noise", "v"}, family
    for family in ("lockstep", "unipc"):
        assert {(bool(v["dp"]), bool(v["p2"])) for v in VARIANTS[family] if v["form"] == "UNIPC"} == set(UNIPC_SHAPES), family
    assert {v["guidance"] for v in VARIANTS["lockstep"]} == {"uncond", "classifier-free"}
    assert any(v.get("blend") for v in VARIANTS["f64"])
    assert THR_BATCHES == (1, 3) and all(n > T and n // T >= 2 for n in THR_CLUSTERED) and any(n % T for n in THR_CLUSTERED)
    for family in FUSED:                                                   # the three parts of a fused test are the cells
        parts = [_fused_cells(family, part) for part in (0, 1, 2)]
        assert set().union(*parts) == set(cells(family)) and sum(len(x) for x in parts) == len(cells(family))
    # per-request stages: the requests that may FUSE are `count` in every whole-group cell (the fall-back requests come on top)
    for (size, count, offset), v in plan("het", 0):
        cases = het_requests(v, size, count, torch.float16, torch.float16, offset, seed=size + count)
        want = count if (offset == 0 and size % G.EPT == 0) else 0
        assert fusable_count(cases) == want and len(cases) == count + (2 if count >= 3 else 0), (size, count, offset)
    assert {v["form"] for v in VARIANTS["lockstep"]} == {"LIN1", "TWO", "MS3", "UNIPC"} and any(v["noise"] for v in VARIANTS["lockstep"])
    assert {v["form"] for v in VARIANTS["het"]} == set(HET_MIX)


# ------------------------------------------------------------------------------------------------
# stage records and cases
# ------------------------------------------------------------------------------------------------
def make_stage(form, guidance="uncond", model="noise", store_m=True, noise=False, thresh=False, blend=False, dp=False, p2=False,
               xc=False, seed=0):
    """a stage record with scalars of realistic magnitude (as the _stage helpers of test_gpu_het.py / test_gpu_unipc.py)"""
    rng = random.Random(seed)
    st = L.Stage()
    st.index, st.form, st.model_type, st.guidance = NOISE_INDEX, _F[form], L.MODEL[model], L.GUIDE[guidance]
    st.flags = L.F_TO_X0 | (L.F_STORE_M if store_m else 0) | (L.F_NOISE if noise else 0) | (L.F_THRESH if thresh else 0) | \
        (L.F_BLEND if blend else 0)
    st.h1_slot = st.h2_slot = st.m_slot = -1
    a = rng.uniform(0.05, 0.999)
    st.alpha_e, st.sigma_e = a, math.sqrt(1.0 - a * a)
    st.cfg_scale = 3.0 if guidance == "classifier-free" else 1.0
    st.cg_scale = 0.7
    st.thr_ratio, st.thr_max = 0.995, 1.0
    a2 = rng.uniform(0.1, 0.99)
    st.blend_alpha, st.blend_sigma = a2, math.sqrt(1.0 - a2 * a2)
    if form == "UNIPC":
        st.flags |= (L.F_UNIPC_DP if dp else 0) | (L.F_UNIPC_P2 if p2 else 0) | (L.F_STORE_XC if xc else 0)
        st.cx, st.c0, st.c1, st.c2 = 0.83 + 0.01 * rng.random(), -0.47 - 0.01 * rng.random(), -0.238, -0.208
        st.k[0], st.k[1], st.k[2] = 0.6685, -0.2782, -0.6686
        return st
    if form == "TWO" and rng.random() < 0.3:
        st.flags |= L.F_BASE_HIST
    st.cx, st.c0, st.c1, st.c2 = (rng.uniform(-2, 2) for _ in range(4))
    for j in range(4):
        st.k[j] = rng.uniform(-1.5, 1.5)
    st.k[4] = rng.uniform(0.5, 1.5)
    return st


def _n_of(v, size):
    return size * v["stride_batch"] if v.get("stride_batch") else size


def _blend_of(v, n):
    """(mask_period, with blend_b, layout) of a blend variant at n elements: the wanted layout where its period divides n, else
    the next one down (split: a multiple of the tile; pack: a multiple of 8 that is not; ragged: anything else)"""
    kind = v["blend"]
    if kind == "split" and n % T != 0:
        kind = "pack"
    if kind == "pack" and n % 8 != 0:
        kind = "ragged"
    if kind == "split":
        return T, v.get("blend_b", True), kind
    if kind == "pack":
        return (24 if n % 24 == 0 and n > 24 else 8), v.get("blend_b", True), kind
    p = next((q for q in (3, 5, 7, 9, 11, 13) if n % q == 0 and n > q), n if n % 8 else 1)
    return p, v.get("blend_b", True), kind


def make_case(family, v, size, sd, ed, offset=0, req=0, seed=0, form=None, per_request=False, store_m=None):
    """the CPU GuardedLaunch of variant v at `size`"""
    form = form or v["form"]
    st = make_stage(form, v["guidance"], v["model"], v["store_m"] if store_m is None else store_m, noise=v.get("noise", False),
                    blend=bool(v.get("blend")), dp=v.get("dp", False), p2=v.get("p2", False), xc=v.get("xc", False),
                    seed=seed * 131 + (req if per_request else 0))
    n, kw = _n_of(v, size), {}
    if v.get("stride_batch"):
        kw.update(batch=v["stride_batch"], stride=2 * size)
    if v.get("blend"):
        kw.update(blend=_blend_of(v, n)[:2])
    return G.GuardedLaunch(family, st, n, sd, ed, offset=offset, dup=v.get("dup", False), sep_xe=v.get("sep_xe", False),
                           seed=seed, req=req, noise_seed=(1000 + req) if st.flags & L.F_NOISE else None,
                           per_request_stages=per_request, **kw)


def het_requests(v, size, count, sd, ed, offset, seed):
    """the requests of one per-request-stage call: `count` requests of `size` elements at `offset` -- forms of the mix in
    rotation, STORE_M mixed -- and, in calls of three or more, two more ON TOP of them that fall back inside the same call:
    one sits one element past its alignment (inserted second), one has a ragged size (appended last)"""
    mix, specs = HET_MIX[v["form"]], [(size, offset)] * count
    if count >= 3:
        specs = specs[:1] + [(size, 1)] + specs[1:] + [(size // 8 * 8 + 3, offset)]
    out = []
    for r, (n, off) in enumerate(specs):
        form = mix[(r + seed) % len(mix)]
        vv = dict(v, form=form, noise=(v["form"] == "noise"), dp=(r % 2 == 0), p2=(r % 3 != 1))
        out.append(make_case("het", vv, n, sd, ed, off, req=r, seed=seed, per_request=True, store_m=(r + seed) % 3 != 0))
    return out


def fusable_count(cases):
    """how many requests of a per-request-stage call the fused kernels may take (dense, whole groups, 16-byte aligned, the
    size of request 0)"""
    return sum(1 for c in cases if c.offset == 0 and c.n % G.EPT == 0 and c.n == cases[0].n)


# ------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_z():
    """SDE doubles take the kernel's own z: one pure-noise launch of NZ elements per (seed, stage index), cached; every
    smaller n reads a prefix (the noise contract: z of element i depends on seed, stage index and i only)"""
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    cache, old = {}, SD.Z_SOURCE[0]

    def z(seed, index, n):
        if (seed, index) not in cache:
            cache[(seed, index)] = kernel_z(seed, index, NZ)
        assert n <= NZ
        return cache[(seed, index)][:n]
    SD.Z_SOURCE[0] = z
    yield z
    SD.Z_SOURCE[0] = old
    torch.cuda.synchronize()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def noise_stage(index):
    """LIN1 + DPM_F_NOISE, x_start network, cx = c0 = 0, c2 = 1: on any finite x and e0, x_out = z exactly"""
    st = L.Stage()
    st.index, st.form, st.flags, st.model_type = index, L.FORM_LIN1, L.F_NOISE, L.MODEL["x_start"]
    st.h1_slot = st.h2_slot = st.m_slot = -1
    st.alpha_e = st.sigma_e = st.cfg_scale = 1.0
    st.c2 = 1.0
    return st


def kernel_z(seed, index, n):
    x, e0, out = (torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(3))
    o = L.LaunchOpts()
    o.noise_seed_lo, o.noise_seed_hi = seed & 0xFFFFFFFF, seed >> 32
    b = L.Buffers()
    b.x, b.e0, b.x_out, b.n, b.batch = x.data_ptr(), e0.data_ptr(), out.data_ptr(), n, 1
    b.state_dtype = b.eps_dtype = L.DTYPE_F32
    b.opts = C.pointer(o)
    L.check(L.lib.dpm_stage_launch(C.byref(noise_stage(index)), C.byref(b), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_single(case):
    want, dev = G.run_double(case), case.on(DEV)
    rc = L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    dev.verify(want)


def run_multi(cases, per_request):
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    R = len(cases)
    arr_b = (L.Buffers * R)(*[d.b for d in devs])
    st = (L.Stage * R)(*[d.st for d in devs]) if per_request else C.byref(devs[0].st)
    rc = L.lib.dpm_stage_launch_multi(st, arr_b, R, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())
    G.verify_all(devs, wants)


def _sweep_single(family, sd, ed, p):
    for (size, _, offset), v in plan(family, p):
        run_single(make_case(family, v, size, sd, ed, offset, seed=size + 7 * offset))


# ------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_single_launch_streaming(p, gpu_z):
    _sweep_single("stream", *PAIRS[p], p)


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_kext(p, gpu_z):
    _sweep_single("kext", *PAIRS[p], p)


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_unipc_single(p, gpu_z):
    _sweep_single("unipc", *PAIRS[p], p)


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_sde_single(p, gpu_z):
    _sweep_single("sde", *PAIRS[p], p)


@gpu
def test_double_states(gpu_z):
    _sweep_single("f64", torch.float64, torch.float64, 0)


@gpu
def test_sde_noise_contract(gpu_z):
    """z of element i is the contract's at i for every size and route: each n -- split tiles, a partial tile, the scalar route
    (ragged n, offset 1) -- against a prefix of one NZ-element launch, which itself sits within 1e-5 of the float64 restatement
    (the bound of test_gpu_sde.py)"""
    seed = 0x0123456789ABCDEF
    big = gpu_z(seed, 5, NZ).astype(np.float64)
    want = SD.noise_z64(seed, 5, NZ)
    assert np.all(np.abs(big - want) <= 1e-5 * np.maximum(1.0, np.abs(want))), float(np.max(np.abs(big - want)))
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        for n, _, offset in cells("sde"):
            case = G.GuardedLaunch("sde-contract", noise_stage(5), n, dt, dt, offset=offset, seed=n, noise_seed=seed)
            run_single(case)


def _fused_cells(family, part):
    """part 0: every size at 1, 3 and 9 requests, and the offset-1 cells; 1: the request counts below 16; 2: 16 and above"""
    pick = {0: lambda i, c: i < 3 * len(SIZES) or c[2] == 1, 1: lambda i, c: i >= 3 * len(SIZES) and c[2] == 0 and c[1] < 16,
            2: lambda i, c: i >= 3 * len(SIZES) and c[2] == 0 and c[1] >= 16}[part]
    return {c for i, c in enumerate(cells(family)) if pick(i, c)}


@gpu
@pytest.mark.parametrize("part", [0, 1, 2])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_lockstep_fused(p, part, gpu_z):
    sd, ed = PAIRS[p]
    mine = _fused_cells("lockstep", part)
    for (size, count, offset), v in plan("lockstep", p):
        if (size, count, offset) in mine:
            run_multi([make_case("lockstep", v, size, sd, ed, offset, req=r, seed=size + count) for r in range(count)], False)


@gpu
@pytest.mark.parametrize("part", [0, 1, 2])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_heterogeneous_fused(p, part, gpu_z):
    sd, ed = PAIRS[p]
    mine = _fused_cells("het", part)
    for (size, count, offset), v in plan("het", p):
        if (size, count, offset) in mine:
            run_multi(het_requests(v, size, count, sd, ed, offset, seed=size + count), True)


def thresh_case(form, guidance, per, batch, sd, ed, req=0, seed=0):
    st = make_stage(form, guidance, "noise", True, thresh=True, seed=seed)
    nb = int(L.lib.dpm_threshold_workspace_bytes(batch, per))
    return G.GuardedLaunch("thresh", st, per * batch, sd, ed, batch=batch, ws_bytes=nb, seed=seed, req=req)


@gpu
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_thresholding(p, gpu_z):
    """DPM_F_THRESH alone and as the multi-request launch (3 requests, each its own workspace arena); a size the library
    rejects must leave every output arena untouched"""
    sd, ed = PAIRS[p]
    i = p
    for per in THR_SIZES + THR_CLUSTERED:
        for batch in THR_BATCHES:
            assert (int(L.lib.dpm_threshold_workspace_bytes(batch, per)) > 0) == (per in THR_CLUSTERED), (per, batch)
            form, guidance = ("LIN1", "TWO", "MS3")[i % 3], ("uncond", "classifier-free")[(i // 3) % 2]
            i += 1
            for count in (1, 3):
                cases = [thresh_case(form, guidance, per, batch, sd, ed, req=r, seed=per + batch) for r in range(count)]
                wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
                arr_b = (L.Buffers * count)(*[d.b for d in devs])
                if count == 1:
                    rc = L.lib.dpm_stage_launch(C.byref(devs[0].st), arr_b, _stream())
                else:
                    rc = L.lib.dpm_stage_launch_multi(C.byref(devs[0].st), arr_b, count, _stream())
                torch.cuda.synchronize()
                G.verify_all(devs, wants, rc)


@gpu
def test_a_call_that_fails_writes_nothing(gpu_z):
    sd = ed = torch.float16
    v = V("TWO")
    dev = make_case("stream", v, T + 8, sd, ed).on(DEV)
    dev.b.h1 = None
    rc = L.lib.dpm_stage_launch(C.byref(dev.st), C.byref(dev.b), _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"needs h1" in L.lib.dpm_last_error()
    dev.verify(rc=rc)
    # per-request stages: every request is checked before anything is launched
    devs = [c.on(DEV) for c in het_requests(V("het3"), T + 8, 4, sd, ed, 0, seed=1)]
    devs[3].st.form, devs[3].b.h1 = L.FORM_TWO, None
    R = len(devs)
    arr_b = (L.Buffers * R)(*[d.b for d in devs])
    rc = L.lib.dpm_stage_launch_multi((L.Stage * R)(*[d.st for d in devs]), arr_b, R, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"needs h1" in L.lib.dpm_last_error()
    G.verify_all(devs, rc=rc)
    # the same stage for every request: requests of different sizes are launched one by one, and still the last request's
    # error is found before the first one is launched
    devs = [make_case("lockstep", v, n, sd, ed, req=r, seed=2).on(DEV) for r, n in enumerate((T + 8, T + 8, 3 * T))]
    devs[2].b.h1 = None
    arr_b = (L.Buffers * 3)(*[d.b for d in devs])
    rc = L.lib.dpm_stage_launch_multi(C.byref(devs[0].st), arr_b, 3, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"needs h1" in L.lib.dpm_last_error()
    G.verify_all(devs, rc=rc)
