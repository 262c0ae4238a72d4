"""The walk of a table-mode call with EVERY row kind in it at once: one DPM_TABLE_FILL | NOISE | THRESH | BLEND call of the real
library through ctypes, no GPU, in the style of tests/test_table_host.py and its three siblings (each of which sets at most two of
the flags).  Plain / UniPC, SDE, thresholded and mask-blend requests are interleaved in call order; the table must hold the runs in
the order their groups open, members in call order, ONE row counter across the kinds, every record at the global row index in its
own section, and nothing else written.  Then the same call with each flag cleared in turn: that kind's requests own no rows, and
without the noise section the blend section starts right behind the rows.  Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

from dpm_solver_amd import _lib as L
from test_table_host import FIELDS, HDR, POISON, ROW

NZ, BL = int(L.lib.dpm_sizeof(10)), int(L.lib.dpm_sizeof(12))
ALL = L.TABLE_NOISE | L.TABLE_THRESH | L.TABLE_BLEND
N = 2048                                   # elements of a plain / SDE request; blend requests have 8, thresholded 2 x 12

# The call, in call order.  plain: LIN1 / TWO alternating; unipc; ms3; sde / sde_v (another model type: a run of its own);
# thr / thr_b (another thr_ratio: a run of its own); blend; ragged (n % 8 != 0).
KINDS = (["plain", "thr", "plain", "sde", "blend", "plain", "unipc", "ms3", "sde_v", "plain", "thr_b", "ragged", "sde", "plain",
          "thr", "blend", "unipc"] + ["plain"] * 12)
PLAIN = [r for r, k in enumerate(KINDS) if k in ("plain", "unipc")]
assert len(KINDS) == 29 and KINDS.count("plain") == 17 and len(PLAIN) == 19 and KINDS.index("unipc") < KINDS.index("ms3")


def where(kind):
    return [r for r, k in enumerate(KINDS) if k == kind]


# the runs a flag word leaves, in the order their groups open: (kind of record, members); the MS3 request (turned away by the
# group that holds UniPC records, alone too small for rows) and the ragged one own no rows under any flag
def runs(flags):
    out = [(0, "plain", PLAIN)]                                                          # opens with request 0
    if flags & L.TABLE_THRESH:
        out.append((1, "thr", where("thr")))
    if flags & L.TABLE_NOISE:
        out.append((3, "sde", where("sde")))
    if flags & L.TABLE_BLEND:
        out.append((4, "blend", where("blend")))
    if flags & L.TABLE_NOISE:
        out.append((8, "sde", where("sde_v")))
    if flags & L.TABLE_THRESH:
        out.append((10, "thr", where("thr_b")))
    assert [o[0] for o in out] == sorted(o[0] for o in out) and all(o[0] == o[2][0] for o in out)
    return [(kind, members) for _, kind, members in out]


class Call:
    """the 29 requests with fabricated, distinct, 16-byte aligned addresses (FILL dereferences none of them)"""

    def __init__(self, noise_base=True):
        R = self.R = len(KINDS)
        self.st, self.bs = (L.Stage * R)(), (L.Buffers * R)()
        self.ropts = [L.LaunchOpts() for _ in range(R)]
        p0 = 1 << 32
        for r, kind in enumerate(KINDS):
            s, b = self.st[r], self.bs[r]
            s.index, s.form = 2 + r, (L.FORM_LIN1, L.FORM_TWO)[r % 2]
            s.flags = L.F_TO_X0 | (L.F_STORE_M if r % 3 else 0)
            s.model_type, s.guidance = L.MODEL["noise"], L.GUIDE["uncond"]
            s.alpha_e, s.sigma_e = 0.75 + 0.001 * r, 0.5 - 0.001 * r
            s.cx, s.c0, s.c1, s.c2 = 0.9, -0.1 - 0.01 * r, 0.05, 0.25 + 0.015625 * r
            s.k[0] = 0.5
            p = [p0 + ((r * 16 + k) << 20) for k in range(12)]
            b.x, b.e0, b.h1, b.h2, b.x_out, b.m_out = p[0], p[1], p[3], p[4], p[5], p[6]
            b.n, b.batch = N, 1
            b.state_dtype = b.eps_dtype = L.DTYPE_F16
            if kind == "unipc":
                s.form, s.flags = L.FORM_UNIPC, s.flags | (L.F_UNIPC_DP if r % 2 else L.F_UNIPC_P2)
            elif kind == "ms3":
                s.form = L.FORM_MS3
            elif kind in ("sde", "sde_v"):
                s.flags |= L.F_NOISE
                self.ropts[r].noise_seed_lo, self.ropts[r].noise_seed_hi = 0x1000 + r, 0xABCD0000 + 7 * r
                b.opts = C.pointer(self.ropts[r])
                b.noise_sample0 = 1 + r % 3 if noise_base else 0
                if kind == "sde_v":
                    s.model_type = L.MODEL["v"]
            elif kind in ("thr", "thr_b"):
                s.form = (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3)[r % 3]
                s.flags |= L.F_THRESH
                s.thr_ratio, s.thr_max = (0.995 if kind == "thr" else 0.99), 1.0
                b.n, b.batch = 24, 2                                   # samples of 12 elements
            elif kind == "blend":
                s.flags |= L.F_BLEND
                s.blend_alpha, s.blend_sigma = 0.25 + 0.0078125 * r, 0.5 - 0.00390625 * r
                b.mask, b.blend_a, b.blend_b = p[8], p[9], (p[10] if r % 2 else None)
                b.n, b.mask_period = 8, 8
            elif kind == "ragged":
                b.n = N - 4
        self.opts = L.LaunchOpts()
        self.opts.per_request_stages = 1
        self.bs[0].opts = C.pointer(self.opts)
        self.size = HDR + R * (ROW + NZ + BL)                          # room for both sections, whatever the flags
        self.table = np.full(self.size + 64 + 16, POISON, dtype=np.uint8)      # 64 guard bytes behind the last record
        self.toff = (-self.table.ctypes.data) % 16
        self.bs[0].workspace = self.table.ctypes.data + self.toff

    def fill(self, flags):
        self.table[:] = POISON
        self.opts.table_mode = L.TABLE_FILL | flags
        rc = L.lib.dpm_stage_launch_multi(self.st, self.bs, self.R, None)
        assert rc == 0, (rc, L.lib.dpm_last_error().decode())
        return self.table[self.toff:self.toff + self.size + 64]

    def want_row(self, r):
        """(the 8 pointers, alpha_e's bits, the flags, the form) of request r's row: the restatement of test_table_host.py"""
        return ([getattr(self.bs[r], f) or 0 for f in FIELDS], int(np.float32(self.st[r].alpha_e).view(np.uint32)),
                self.st[r].flags, self.st[r].form)

    def want_noise(self, r):
        g0 = self.bs[r].noise_sample0 * (self.bs[r].n // self.bs[r].batch) // 4
        return [self.ropts[r].noise_seed_lo, self.ropts[r].noise_seed_hi, self.st[r].index,
                int(np.float32(self.st[r].c2).view(np.uint32)), g0 & 0xffffffff, g0 >> 32, 0, 0]

    def want_blend(self, r):
        s, b = self.st[r], self.bs[r]
        return ([b.mask, b.blend_a, b.blend_b or 0, b.mask_period],
                [int(np.float32(v).view(np.uint32)) for v in (s.blend_alpha, s.blend_sigma)] + [0, 0])


def check(c, flags):
    got = c.fill(flags)
    want = runs(flags)
    order = [r for _, members in want for r in members]
    assert [int(v) for v in got[:HDR].view(np.uint32)] == [L.TABLE_MAGIC, L.lib.dpm_version(), c.R, len(want)]
    owned = np.zeros(len(got), dtype=bool)
    owned[:HDR] = True
    noise0 = HDR + c.R * ROW                                           # the noise section: there iff the flag is
    blend0 = noise0 + (c.R * NZ if flags & L.TABLE_NOISE else 0)       # the blend section: behind it
    kinds = [kind for kind, members in want for _ in members]
    for i, (r, kind) in enumerate(zip(order, kinds)):                  # i: the global row index
        lo = HDR + i * ROW
        row = got[lo:lo + ROW].copy()
        words = row[64:].view(np.uint32)
        assert (row[:64].view(np.uint64).tolist(), int(words[0]), int(words[1]), int(words[5])) == c.want_row(r), (i, r)
        owned[lo:lo + ROW] = True
        if kind == "sde":
            lo = noise0 + i * NZ
            assert got[lo:lo + NZ].copy().view(np.uint32).tolist() == c.want_noise(r), (i, r)
            owned[lo:lo + NZ] = True
        elif kind == "blend":
            lo = blend0 + i * BL
            rec = got[lo:lo + BL].copy()
            assert (rec[:32].view(np.uint64).tolist(), rec[32:].view(np.uint32).tolist()) == c.want_blend(r), (i, r)
            owned[lo:lo + BL] = True
    # rows behind the last run, the record slots of rows that own no record of that kind, a section the flags leave out, the
    # guard bytes: all as they were
    assert (got[~owned] == POISON).all(), np.flatnonzero((got != POISON) & ~owned)[:8]
    return order


def test_every_kind_in_one_call():
    c = Call()
    order = check(c, ALL)
    # the groups in the order they open, members in call order: 19 plain / UniPC rows, then both kinds of thresholded, SDE and
    # blend runs as their first members come up
    assert order == PLAIN + [1, 14, 3, 12, 4, 15, 8, 10] and len(runs(ALL)) == 6
    assert {c.st[r].form for r in PLAIN} == {L.FORM_LIN1, L.FORM_TWO, L.FORM_UNIPC}
    assert (HDR, ROW, NZ, BL) == (16, 144, 32, 48)


@pytest.mark.parametrize("cleared", ["NOISE", "THRESH", "BLEND"])
def test_a_cleared_flag_takes_its_kind_out_of_the_table(cleared):
    flag = getattr(L, "TABLE_" + cleared)
    # (without DPM_TABLE_NOISE a non-zero noise_sample0 is an argument error: that call's SDE requests carry none)
    c = Call(noise_base=cleared != "NOISE")
    order = check(c, ALL & ~flag)
    gone = {"NOISE": where("sde") + where("sde_v"), "THRESH": where("thr") + where("thr_b"), "BLEND": where("blend")}[cleared]
    assert not set(order) & set(gone) and len(order) == 27 - len(gone)
    if cleared == "NOISE":                                             # the blend records: right behind the rows, at rows 21 and 22
        assert order.index(4) == 21 and order.index(15) == 22
