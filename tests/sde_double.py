"""numpy double of the SDE stage (DPM_F_NOISE) -- TEST INFRASTRUCTURE, never imported by the product.

`philox4x32_10` / `noise_z` restate the noise contract of include/dpm_hip.h (Philox4x32-10, Box-Muller, element i of the flat
[B, C, H, W] order); `launch_raw_noise_double` is the pointer-level double of dpm_stage_launch for a noise stage, composed of
kernel_double.py's functions: the update in fp32, + c2 * z (one product, one sum), one rounding to the state dtype.
`install_sde_double` puts it behind the prebuilt launch records on top of kernel_double.install_cpu_double.  `Z_SOURCE` may
be replaced by a function (seed, stage index, n) -> fp32 z, e.g. the kernel's own z taken by a pure-noise launch.
"""
import numpy as np

import kernel_double as KD
from dpm_solver_amd import _lib as L

_MASK = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit values, key: 2 ints -> the 4 output words as uint64 arrays (Random123)"""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in ctr]
    k0, k1 = np.uint64(key[0]) & _MASK, np.uint64(key[1]) & _MASK
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def unit(r):
    """u = ((r >> 9) + 0.5) * 2^-23 (exact in fp32; returned as float64)"""
    return ((r >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def philox_words(seed, index, n):
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    return philox4x32_10((g & _MASK, g >> np.uint64(32), np.full_like(g, index & 0xFFFFFFFF), np.zeros_like(g)),
                         (seed & 0xFFFFFFFF, seed >> 32))


def noise_z64(seed, index, n):
    """the z of elements 0 .. n-1 in float64 (Box-Muller in double on the contract's u)"""
    r = philox_words(seed, index, n)
    rad0, rad1 = np.sqrt(-2.0 * np.log(unit(r[0]))), np.sqrt(-2.0 * np.log(unit(r[2])))
    a1, a3 = 2.0 * np.pi * unit(r[1]), 2.0 * np.pi * unit(r[3])
    z = np.stack([rad0 * np.cos(a1), rad0 * np.sin(a1), rad1 * np.cos(a3), rad1 * np.sin(a3)], axis=1).reshape(-1)
    return z[:n]


Z_SOURCE = [lambda seed, index, n: noise_z64(seed, index, n).astype(np.float32)]


def _seed_of(b):
    o = b.opts.contents if b.opts else None
    return 0 if o is None else (int(o.noise_seed_lo) | (int(o.noise_seed_hi) << 32))


def launch_raw_noise_double(st_ref, b_ref, stream):
    st, b = st_ref._obj, b_ref._obj
    if not (st.flags & L.F_NOISE):
        return KD.launch_raw_double(st_ref, b_ref, stream)
    n, sd, ed = int(b.n), b.state_dtype, b.eps_dtype
    assert not b.eps_stride and not (st.flags & (L.F_THRESH | L.F_BLEND)), "not restated for SDE stages"
    x, xe = KD._rd(b.x, n, sd), KD._rd(b.xe, n, sd)
    if xe is None:
        xe = x
    c = KD._Coef(st)
    mn = KD.prologue(c, xe, KD._rd(b.e0, n, ed), KD._rd(b.e1, n, ed), KD._rd(b.g, n, ed), KD.half_rounder(ed))
    out = KD.combine(c, x, mn, KD._rd(b.h1, n, sd), KD._rd(b.h2, n, sd), KD.half_rounder(ed)).astype(np.float32)
    z = np.asarray(Z_SOURCE[0](_seed_of(b), int(st.index), n), dtype=np.float32)
    out = (out + (np.float32(st.c2) * z).astype(np.float32)).astype(np.float32)
    KD._wr(b.x_out, out, sd)
    if b.x_out2:
        KD._wr(b.x_out2, out, sd)
    if st.flags & L.F_STORE_M:
        KD._wr(b.m_out, mn, sd)
    return 0


def install_sde_double(monkeypatch, S, D):
    """kernel_double.install_cpu_double + the noise stage behind the prebuilt launch records (sample_sde's fast path)"""
    KD.install_cpu_double(monkeypatch, S, D)
    monkeypatch.setattr(S, "_stage_launch_raw", launch_raw_noise_double)


def buffers_ref(b):
    """(ctypes.byref stand-in) for calling launch_raw_noise_double on a Buffers built by hand"""
    return KD._Ref(b)

