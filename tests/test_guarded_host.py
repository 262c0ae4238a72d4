"""The guard-band helper (tests/guarded.py) must be shown to fail -- CPU only.

First the numpy doubles themselves run through the arenas over the whole size list of tests/test_gpu_edges.py (which also
bounds-checks the doubles).  Then fake launchers -- plain Python writing through the same raw pointers: a double plus one
defect each -- must make `verify()` raise with the right buffer named.  Nothing here touches a GPU.
"""
import numpy as np
import pytest
import torch

import guarded as G
import kernel_double as KD
import test_gpu_edges as E
from dpm_solver_amd import _lib as L

T = G.T
F16, F32 = torch.float16, torch.float32


def test_fill_patterns_are_nans_no_update_produces():
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        es = torch.empty(0, dtype=dt).element_size()
        v = torch.tensor([G.FILL[es]], dtype=G._INT[es]).view(dt)
        assert bool(torch.isnan(v).all())
        canonical = (torch.zeros(1, dtype=dt) / torch.zeros(1, dtype=dt)).view(G._INT[es])
        assert int(canonical) != G.FILL[es] and int((-(canonical.view(dt))).view(G._INT[es])) != G.FILL[es]
    a = G.Arena(torch.float16, 9, "cpu", offset=1)
    assert (a.ptr - 2) % 16 == 0 and a.lead >= G.GUARD and a.raw.numel() - a.lead - a.extent >= G.GUARD


@pytest.mark.parametrize("family", sorted(E.VARIANTS))
def test_doubles_stay_inside_their_payloads(family):
    """every variant of every family at every size (single-launch cells; per-request cells at 3 requests), fp32 and fp16"""
    pairs = [(torch.float64, torch.float64)] if family == "f64" else [(F32, F32), (F16, F16)]
    for sd, ed in pairs:
        for i, size in enumerate(E.SIZES):
            for offset in ((0, 1) if size in E.OFFSET1 else (0,)):
                vs = E.VARIANTS[family]
                for v in (vs if size in E.OFFSET1 else vs[i % 3::3]):
                    if family == "het":
                        for c in E.het_requests(v, size, 3, sd, ed, offset, seed=size):
                            G.run_double(c)
                    else:
                        G.run_double(E.make_case(family, v, size, sd, ed, offset, seed=size))


def test_threshold_doubles_stay_inside_their_payloads():
    for per in E.THR_SIZES + E.THR_CLUSTERED:
        for batch in E.THR_BATCHES:
            c = G.run_double(E.thresh_case("TWO", "uncond", per, batch, F32, F32, seed=per))
            assert bool((c.arenas["x_out"].payload().abs() < 1e3).all())


def test_blend_in_the_pointer_level_double_equals_the_tensor_level_double():
    v = E.V("TWO", blend="pack", model="noise")
    for sd in (F32, F16):
        c = G.run_double(E.make_case("kext", v, 3 * T + 8, sd, sd, seed=3))
        A = {k: a.payload() for k, a in c.arenas.items() if a.extent}
        A = {k: (t if k == "mask" else t.reshape(-1, 8)) for k, t in A.items()}      # a [8] mask broadcast over [n / 8, 8]
        ext = dict(blend=(A["mask"], 8, A["blend_a"], A["blend_b"], c.st.blend_alpha, c.st.blend_sigma))
        x_out, m = KD.launch_stage_double(c.st, A["x"], None, A["e0"], None, None, A["h1"], None, sd, ext=ext)
        bits = lambda t: t.view(G._INT[t.element_size()])
        assert torch.equal(bits(x_out), bits(A["x_out"])) and torch.equal(bits(m), bits(A["m_out"]))


# ------------------------------------------------------------------------------------------------
# fake launchers: the double, then one defect written through the same pointers
# ------------------------------------------------------------------------------------------------
def _case(n=T + 8, sd=F16, store_m=True, req=0):
    return E.make_case("fake", E.V("TWO", store_m=store_m), n, sd, sd, req=req, seed=5)


def _es(c):
    return c.arenas["x_out"].es


def _refill(c, name, lo, hi):
    a = c.arenas[name]
    G.poke(a.ptr + lo * a.es, np.full(hi - lo, G.FILL[a.es]), a.es)


def past_the_end(c):
    G.poke(c.b.x_out + c.n * _es(c), [0x3C00], _es(c))


def before_the_start(c):
    G.poke(c.b.x_out - _es(c), [0x3C00], _es(c))


def m_out_without_store_m(c):
    KD._wr(c.b.m_out, np.ones(c.n, dtype=np.float32), G.CODE[c.sd])


def input_changed(c):
    G.poke(c.b.h1 + 5 * _es(c), [0x3C00], _es(c))


def last_group_not_stored(c):
    _refill(c, "x_out", c.n - 8, c.n)


def last_tile_in_the_split_layouts_second_half(c):
    """the incomplete last tile [T, T + 8) stored 1024 elements further on, where the second half of a split tile goes"""
    es = _es(c)
    tail = G.peek(c.b.x_out + T * es, c.n - T, es)
    _refill(c, "x_out", T, c.n)
    G.poke(c.b.x_out + (T + 1024) * es, tail, es)


DEFECTS = [(past_the_end, True, "x_out", T + 8), (before_the_start, True, "x_out", -1), (m_out_without_store_m, False, "m_out", 0),
           (input_changed, True, "h1", 5), (last_group_not_stored, True, "x_out", T),
           (last_tile_in_the_split_layouts_second_half, True, "x_out", None)]


@pytest.mark.parametrize("defect,store_m,buffer,offset", DEFECTS, ids=[d[0].__name__ for d in DEFECTS])
@pytest.mark.parametrize("sd", [F16, F32], ids=["f16", "f32"])
def test_a_seeded_defect_is_detected(defect, store_m, buffer, offset, sd):
    want = G.run_double(_case(sd=sd, store_m=store_m))
    got = _case(sd=sd, store_m=store_m)
    assert G.double_launch(got.st, got.b) == 0
    got.verify(want)                                     # the double alone passes
    defect(got)
    with pytest.raises(G.GuardError) as e:
        got.verify(want)
    msg = str(e.value)
    assert "family=fake" in msg and "pair=%s/%s" % (G._name(sd), G._name(sd)) in msg and "n=%d" % (T + 8) in msg
    assert "request=0" in msg and "buffer=%s " % buffer in msg, msg
    if offset is not None:
        assert "offset=%d:" % offset in msg, msg


def test_a_super_tile_written_into_the_next_requests_buffer_is_detected():
    wants = [G.run_double(_case(n=3 * T, req=r)) for r in range(3)]
    gots = [_case(n=3 * T, req=r) for r in range(3)]
    for g in gots:
        assert G.double_launch(g.st, g.b) == 0
    G.verify_all(gots, wants)
    es = _es(gots[0])
    G.poke(gots[1].b.x_out, G.peek(gots[0].b.x_out, T, es), es)          # request 0's first tile lands in request 1 ...
    with pytest.raises(G.GuardError, match=r"request=1 buffer=x_out offset=\d+: value differs"):
        G.verify_all(gots, wants)
    _refill(gots[0], "x_out", 0, T)                                        # ... and request 0 never gets it
    with pytest.raises(G.GuardError, match="request=0 buffer=x_out offset=0: payload element still holds the fill"):
        G.verify_all(gots, wants)


def test_an_error_code_must_leave_the_outputs_untouched():
    got = _case()
    got.verify(rc=-1)                                    # nothing ran: passes
    assert G.double_launch(got.st, got.b) == 0
    with pytest.raises(G.GuardError, match="buffer=x_out offset=0: changed by a launch that returned the error code -1"):
        got.verify(rc=-1)


def test_a_wrong_bit_and_a_dirty_workspace_are_detected():
    want, got = G.run_double(_case(sd=F32)), _case(sd=F32)
    assert G.double_launch(got.st, got.b) == 0
    G.poke(got.b.x_out + 4 * 100, G.peek(got.b.x_out + 4 * 100, 1, 4) ^ 1, 4)
    with pytest.raises(G.GuardError, match="buffer=x_out offset=100: value differs"):
        got.verify(want)
    c = G.run_double(E.thresh_case("LIN1", "uncond", 256, 3, F32, F32))
    G.poke(c.arenas["workspace"].ptr - 4, [0], 4)
    with pytest.raises(G.GuardError, match="buffer=workspace offset=-1: guard"):
        c.verify()
