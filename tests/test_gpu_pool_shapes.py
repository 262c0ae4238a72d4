"""Requests of different shapes in one fused launch (dpm_launch_opts.fuse_shapes, stage_kernel_shapes / _shapes_noise /
_shapes_unipc), on the MI355X.  Kernel level, through the C ABI and between guards (tests/guarded.py): per-request-stage calls
whose members take their element counts in rotation from sizes around the tile edges must give every request the bits of its
own dpm_stage_launch AND of the numpy double; the launches are counted by kernel name.  End to end: a staggered
request_pool(mixed_shapes=True) of six shapes against sample / sample_unipc / sample_sde, bit for bit.
Run on an MI355X:  pytest -m gpu
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_amd as D
import guarded as G
import sde_double as SD
import test_gpu_edges as E
from dpm_solver_amd import _lib as L
from test_gpu_edges import PAIRS, PAIR_IDS
from test_gpu_unipc_pool import _stage_kernels

gpu = pytest.mark.gpu
DEV = "cuda:0"
NS = [8, 2040, 2048, 2056, 4096, 4104, 6152, 16384]          # elements of a member, taken in rotation
COUNTS = [2, 3, 9, 16, 17, 33]
# the four mixes (forms in rotation; UNIPC in its four sub-shapes, r % 2 / r % 3) x guidance x prologue (noise: compile-time,
# v: generic)
MIXES = {"het2": ("LIN1", "TWO"), "het3": ("LIN1", "TWO", "MS3"), "unipc": ("UNIPC", "LIN1", "UNIPC", "TWO", "UNIPC", "UNIPC"),
         "noise": ("LIN1", "TWO")}
COMBOS = [(mix, g, m) for g in ("uncond", "classifier-free") for m in ("noise", "v") for mix in MIXES]
PER_CASE = 3                                                  # combos per (dtype pair, request count), in rotation


def combos_of(p, ci):
    """the combos of dtype pair p at request count COUNTS[ci]: 18 consecutive slots per pair cover all 16"""
    return [COMBOS[(PER_CASE * (p * len(COUNTS) + ci) + j) % len(COMBOS)] for j in range(PER_CASE)]


def test_table_covers_every_mix_guidance_and_prologue_per_dtype_pair():
    assert len(COMBOS) == 16 and PAIRS is E.PAIRS and len(PAIRS) == 5
    for p in range(len(PAIRS)):
        assert {c for ci in range(len(COUNTS)) for c in combos_of(p, ci)} == set(COMBOS)
    for ci in range(len(COUNTS)):                             # every request count meets every mix
        assert {c[0] for p in range(len(PAIRS)) for c in combos_of(p, ci)} == set(MIXES), COUNTS[ci]
    # the rotation puts members on either side of the prefix entries and of the XCD span: with 8 sizes of 1 .. 8 tiles and
    # spans of total / 8, some member straddles a span boundary in every call of 9 requests or more
    for count in COUNTS[2:]:
        for u in (1, 2):
            tiles = [-(-(-(-(NS[r % len(NS)] // 8) // 256)) // u) for r in range(count)][:16]
            first = np.cumsum([0] + tiles)
            span = -(-int(first[-1]) // 8)
            assert any(first[r] < k * span < first[r + 1] for r in range(len(tiles)) for k in range(1, 8)), (count, u)


@pytest.fixture(scope="module")
def gpu_z():
    """test_gpu_edges.gpu_z at this file's largest member: the SDE doubles take the kernel's own z, one pure-noise launch of
    max(NS) elements per (seed, stage index), cached (the noise contract: z of element i depends on seed, stage index, i)"""
    assert torch.cuda.is_available(), "these tests need a GPU; run with -m 'not gpu' elsewhere"
    cache, old = {}, SD.Z_SOURCE[0]

    def z(seed, index, n):
        if (seed, index) not in cache:
            cache[(seed, index)] = E.kernel_z(seed, index, max(NS))
        assert n <= max(NS)
        return cache[(seed, index)][:n]
    SD.Z_SOURCE[0] = z
    yield z
    SD.Z_SOURCE[0] = old
    torch.cuda.synchronize()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def requests(mix, guidance, model, count, sd, ed, start=0, seed=0, sizes=None, offsets=None):
    """the CPU cases of one call: request r has NS[(start + r) % 8] elements (or sizes[r]), the mix's forms in rotation, its
    own coefficients and STORE_M bit; an SDE request its own seed and stage index"""
    forms, out = MIXES[mix], []
    for r in range(count):
        n = sizes[r] if sizes else NS[(start + r) % len(NS)]
        v = dict(form=forms[r % len(forms)], guidance=guidance, model=model, store_m=True, noise=(mix == "noise"),
                 dp=(r % 2 == 0), p2=(r % 3 != 1), dup=(guidance != "uncond"))
        c = E.make_case("shapes", v, n, sd, ed, offsets[r] if offsets else 0, req=r, seed=seed, per_request=True,
                        store_m=(r + seed) % 3 != 0)
        if mix == "noise":
            c.st.index = 1 + r % 4
        out.append(c)
    return out


def launch_multi(devs, fuse_shapes=1):
    R = len(devs)
    devs[0].opts.fuse_shapes = fuse_shapes
    arr_b = (L.Buffers * R)(*[d.b for d in devs])
    st = (L.Stage * R)(*[d.st for d in devs])
    rc = L.lib.dpm_stage_launch_multi(st, arr_b, R, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lib.dpm_last_error())


def check_call(cases, what):
    """one fuse_shapes call on guarded operands: guards, inputs and bits against the double (verify), then every request's
    own dpm_stage_launch into the same, refilled, output arenas: the same bits"""
    wants, devs = [G.run_double(c) for c in cases], [c.on(DEV) for c in cases]
    launch_multi(devs)
    G.verify_all(devs, wants)
    for r, d in enumerate(devs):
        fused = {k: d.arenas[k].raw.clone() for k in G.OUTPUTS}
        for k in G.OUTPUTS:
            d.arenas[k].raw.fill_(G.FILL[d.arenas[k].es])
        d.opts.fuse_shapes = 0
        rc = L.lib.dpm_stage_launch(C.byref(d.st), C.byref(d.b), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.dpm_last_error())
        for k in G.OUTPUTS:
            assert torch.equal(fused[k], d.arenas[k].raw), (what, r, d.n, k, "differs from the request's own dpm_stage_launch")
    return devs


@gpu
@pytest.mark.parametrize("ci", range(len(COUNTS)), ids=["%dreq" % c for c in COUNTS])
@pytest.mark.parametrize("p", range(len(PAIRS)), ids=PAIR_IDS)
def test_mixed_shape_calls_equal_the_single_launches_and_the_double(p, ci, gpu_z):
    sd, ed = PAIRS[p]
    for j, (mix, guidance, model) in enumerate(combos_of(p, ci)):
        cases = requests(mix, guidance, model, COUNTS[ci], sd, ed, start=p + ci + 3 * j, seed=7 * p + ci + j)
        check_call(cases, (mix, guidance, model))


def _names(devs, fuse_shapes):
    launch_multi(devs, fuse_shapes)                    # (first-launch costs outside the profile)
    return _stage_kernels(lambda: launch_multi(devs, fuse_shapes))


@pytest.mark.parametrize("sdt", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("mix,family", [("het2", "stage_kernel_shapes<"), ("het3", "stage_kernel_shapes<"),
                                        ("unipc", "stage_kernel_shapes_unipc"), ("noise", "stage_kernel_shapes_noise")])
@gpu
def test_a_mixed_group_is_one_launch_of_the_new_family(sdt, mix, family, gpu_z):
    """kernels counted, not bits: up to 16 requests of different n are ONE launch, 17 are two (the last request's own)"""
    for count, launches in ((3, 1), (16, 1), (17, 2)):
        devs = [c.on(DEV) for c in requests(mix, "uncond", "noise", count, sdt, sdt, start=count)]
        names = _names(devs, 1)
        assert len(names) == launches and sum(family in n for n in names) == 1, (count, names)
        assert sum("stage_kernel_shapes" in n for n in names) == 1, (count, names)


@gpu
def test_without_the_flag_and_with_one_shape_nothing_changes(gpu_z):
    sdt = torch.float16
    devs = [c.on(DEV) for c in requests("het2", "uncond", "noise", 16, sdt, sdt)]
    names = _names(devs, 0)                            # the parent's grouping: one stage_kernel_het launch per n (8 here)
    assert len(names) == len(NS) and all("stage_kernel_het<" in n for n in names), names
    assert not any("stage_kernel_shapes" in n for n in names), names
    assert sum("stage_kernel_shapes" in n for n in _names(devs, 1)) == 1
    for mix, family in (("het2", "stage_kernel_het<"), ("unipc", "stage_kernel_het_unipc"), ("noise", "stage_kernel_het_noise")):
        devs = [c.on(DEV) for c in requests(mix, "uncond", "noise", 9, sdt, sdt, sizes=[4104] * 9)]
        names = _names(devs, 1)                        # fuse_shapes with one n: today's kernels
        assert len(names) == 1 and family in names[0] and "stage_kernel_shapes" not in names[0], (mix, names)
    # one n, two batch sizes: without the flag two groups, with it one launch of today's kernel (it never reads batch)
    cases = requests("het2", "uncond", "noise", 6, sdt, sdt, sizes=[4096] * 6)
    for r, c in enumerate(cases):
        c.batch = c.kw["batch"] = 1 + r % 2
        c.b = c.buffers()
    devs = [c.on(DEV) for c in cases]
    assert len(_names(devs, 0)) == 2
    names = _names(devs, 1)
    assert len(names) == 1 and "stage_kernel_het<" in names[0], names


@gpu
@pytest.mark.parametrize("mix", ["het2", "unipc", "noise"])
def test_members_the_fused_family_does_not_take_fall_back_in_the_same_call(mix, gpu_z):
    """a member with n % 8 != 0 and one that sits one element past its alignment come out right, the other five fuse"""
    sdt = torch.float16
    sizes, offsets = [2048, 2059, 4096, 8, 6152, 16384, 4104], [0, 0, 1, 0, 0, 0, 0]
    for guidance in ("uncond", "classifier-free"):
        cases = requests(mix, guidance, "noise", len(sizes), sdt, sdt, sizes=sizes, offsets=offsets, seed=5)
        devs = check_call(cases, ("fall back", mix, guidance))
        names = _names(devs, 1)
        assert len(names) == 3 and sum("stage_kernel_shapes" in n for n in names) == 1, names


# ---- the pool ---------------------------------------------------------------------------------------------------------
SHAPES = [(1, 4, 8, 8), (2, 4, 16, 16), (3, 4, 16, 16), (2, 4, 32, 32), (1, 3, 24, 24), (1, 3, 5, 5)]
# (tick of admission, shape index, kind, kwargs): the CPU scenario of tests/test_pool_shapes_host.py
MIX = [
    (0, 0, "2m", dict(steps=6, order=2)),
    (0, 1, "unipc", dict(steps=7)),
    (0, 2, "sde", dict(steps=5, seed=0xDEADBEEF12345)),
    (1, 3, "ms3", dict(steps=8, order=3)),
    (1, 4, "2m", dict(steps=4, order=2, skip_type="logSNR")),
    (2, 5, "unipc", dict(steps=5, variant="bh1")),
    (2, 0, "sde", dict(steps=6, seed=3)),
    (3, 1, "ms3", dict(steps=7, order=3, lower_order_final=False)),
    (3, 2, "2m", dict(steps=9, order=2)),
    (5, 3, "unipc", dict(steps=3, order=2)),
    (5, 4, "sde", dict(steps=4, seed=11, order=1)),
    (6, 5, "ms3", dict(steps=6, order=3)),
]
SUBMIT = {"2m": lambda p, x, kw: p.submit(x, **kw), "ms3": lambda p, x, kw: p.submit(x, **kw),
          "unipc": lambda p, x, kw: p.submit_unipc(x, **kw), "sde": lambda p, x, kw: p.submit(x, sde=True, **kw)}


def _solver(cfg, continuous):
    if continuous:
        ns = D.NoiseScheduleVP("linear")         # (a half state stays half on a continuous schedule with a noise network)
    else:
        betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
        ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    if cfg:
        def net(x, t, c):       # c = [uncond, cond], one entry per half of the [2B, ...] input, whatever B
            w = c.repeat_interleave(x.shape[0] // c.shape[0]).reshape(-1, 1, 1, 1)
            return ((0.5 * x.float() + 0.1 * torch.sin(x.float())) * (0.8 + 0.2 * w)).to(x.dtype)
        c = torch.ones(1, device=DEV)
        fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=3.0, condition=c,
                             unconditional_condition=c * 0)
    else:
        fn = D.model_wrapper(lambda x, t: (0.5 * x.float() + 0.1 * torch.sin(x.float())).to(x.dtype), ns)
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")


@gpu
@pytest.mark.parametrize("cfg", [False, True], ids=["uncond", "cfg"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_staggered_pool_of_six_shapes_equals_every_request_alone(dtype, cfg):
    dpm = _solver(cfg, continuous=dtype is torch.float16)
    g = torch.Generator(device=DEV).manual_seed(207)
    xs = [torch.randn(SHAPES[s], generator=g, device=DEV).to(dtype) for _, s, _, _ in MIX]
    pool = dpm.request_pool(mixed_shapes=True)
    handles, got, tick = {}, {}, 0
    while tick <= max(m[0] for m in MIX) or pool:
        for j, (t, _, k, kw) in enumerate(MIX):
            if t == tick:
                handles[SUBMIT[k](pool, xs[j], kw)] = j
        for h, out in pool.step().items():
            got[handles[h]] = out
        tick += 1
    assert sorted(got) == list(range(len(MIX)))
    alone = {"2m": dpm.sample, "ms3": dpm.sample, "unipc": dpm.sample_unipc, "sde": dpm.sample_sde}
    for j, (x, (_, _, k, kw)) in enumerate(zip(xs, MIX)):
        want = alone[k](x, **kw)
        assert got[j].shape == x.shape and got[j].dtype == want.dtype == dtype, (j, k, kw)
        assert torch.equal(got[j], want), (j, k, kw)


@gpu
def test_a_tick_of_six_shapes_is_one_launch():
    dpm = _solver(False, continuous=True)
    g = torch.Generator(device=DEV).manual_seed(3)
    pool = dpm.request_pool(mixed_shapes=True)
    shapes = SHAPES[:5] + [(4, 4, 32, 32)]                  # six shapes of whole 8-element groups
    xs = [torch.randn(s, generator=g, device=DEV).half() for s in shapes]
    hs = [pool.submit(x, steps=5 + j % 2, order=2) for j, x in enumerate(xs)]
    done = dict(pool.step())                                # (first-launch costs outside the profile)
    names = []
    for _ in range(3):
        assert len(pool) == 6
        names.append(_stage_kernels(lambda: done.update(pool.step())))
    assert all(len(n) == 1 and "stage_kernel_shapes<" in n[0] for n in names), names
    while pool:
        done.update(pool.step())
    for j, (h, x) in enumerate(zip(hs, xs)):
        assert torch.equal(done[h], dpm.sample(x, steps=5 + j % 2, order=2)), j
    default = dpm.request_pool()
    default.submit(xs[0], steps=3)
    with pytest.raises(ValueError, match="does not match the pool's"):
        default.submit(xs[1], steps=3)
