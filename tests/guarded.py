"""guard-banded operands of a stage launch -- TEST INFRASTRUCTURE, never imported by the product.

Every operand of a launch (inputs, outputs, the thresholding workspace) lives in an arena of its own:
`guard + extent + guard` elements, the guards and every output payload pre-filled with a NaN bit pattern no update can
produce (the arithmetic of finite inputs yields the canonical quiet NaN at worst, never this payload).  The pattern is
compared as integers.  `GuardedLaunch` builds the `dpm_buffers` record of one request on CPU tensors (for the numpy
doubles, which write through the same raw pointers) and on GPU tensors alike; `verify()` after a launch asserts

  1. every output guard is untouched,
  2. every input arena -- guards and payload -- is byte-identical to its state before the launch,
  3. an output the stage must not write (m_out without DPM_F_STORE_M, an x_out2 the record does not name) is untouched,
  4. every payload element of a written output no longer holds the fill pattern,
  5. the values: bit-equal to the double (2- and 4-byte states); double states within the bound
     tests/test_gpu_parity.py::test_double_precision_state_on_the_gpu applies, 1e-14 of the tensor's scale,
  6. after a call that returned an error code, every output arena is untouched.
"""
import ctypes as C

import numpy as np
import torch

import kernel_double as KD
import sde_double as SD
import unipc_double as UD
from dpm_solver_amd import _lib as L

EPT, T = 8, 2048                 # elements per lane group, elements per tile (256 lanes x EPT)
GUARD = 8192                     # two super-tiles of the widest launch shape (U = 2 tiles x 2048), each side
F64_BOUND = 1e-14                # of max |want|: the bound test_gpu_parity.py applies to double states
CODE = {torch.float16: L.DTYPE_F16, torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float64: L.DTYPE_F64}
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
FILL = {2: 0x7FA5, 4: 0x7FA5C3D2, 8: 0x7FF5A5C3D2E1F0B7}        # NaNs of fp16 / bf16, fp32, fp64 with a payload of their own
INPUTS = ("x", "xe", "e0", "e1", "g", "h1", "h2", "mask", "blend_a", "blend_b")
OUTPUTS = ("x_out", "m_out", "x_out2")


class GuardError(AssertionError):
    pass


def _name(dt):
    return str(dt).split(".")[-1]


class Arena:
    """guard | payload | guard of one operand; the payload starts 16-byte aligned, or `offset` elements further in"""

    def __init__(self, dtype, extent, device, offset=0, bits=None, zero=False):
        self.dtype, self.extent, self.offset = dtype, int(extent), offset
        self.es = es = torch.empty(0, dtype=dtype).element_size()
        a = 16 // es
        self.raw = torch.empty(2 * GUARD + offset + self.extent + a, dtype=_INT[es], device=device)
        self.raw.fill_(FILL[es])
        assert self.raw.data_ptr() % es == 0
        self.lead = GUARD + (-(self.raw.data_ptr() // es)) % a + offset
        assert (self.ptr - offset * es) % 16 == 0 and self.lead >= GUARD and self.raw.numel() - self.lead - self.extent >= GUARD
        if bits is not None:
            self.payload_bits().copy_(bits)
        elif zero:
            self.payload_bits().zero_()
        self.before = self.raw.cpu().clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.lead * self.es

    def payload_bits(self):
        return self.raw[self.lead:self.lead + self.extent]

    def payload(self):
        """the payload as a CPU tensor of the arena's dtype"""
        return self.payload_bits().cpu().view(self.dtype) if self.dtype.is_floating_point else self.payload_bits().cpu()

    def verify(self, what, want_bits=None):
        """an arena outside a GuardedLaunch: both guards as they were, and the payload -- bit for bit -- `want_bits`
        (None: as it was at construction, i.e. nothing wrote it)"""
        now, end = self.raw.cpu(), self.lead + self.extent
        for lo, hi in ((0, self.lead), (end, now.numel())):
            d = now[lo:hi] != self.before[lo:hi]
            if bool(d.any()):
                raise GuardError("%s offset=%d: guard element overwritten" % (what, lo + _first(d) - self.lead))
        want = self.before[self.lead:end] if want_bits is None else want_bits.cpu().reshape(-1)
        d = now[self.lead:end] != want
        if bool(d.any()):
            i = _first(d)
            raise GuardError("%s offset=%d: payload holds bits %#x, want %#x%s" % (
                what, i, int(now[self.lead + i]) & (2 ** (8 * self.es) - 1), int(want[i]) & (2 ** (8 * self.es) - 1),
                " (nothing may write it)" if want_bits is None else ""))


def _first(mask):
    return int(torch.nonzero(mask.reshape(-1))[0])


class GuardedLaunch:
    """the operands of one request of one launch, each in a guarded arena, and its dpm_buffers record.

    st: the L.Stage (decides which operands exist: h1 / h2 by form, e1 under classifier-free guidance, g under classifier
    guidance, mask / blend_a / blend_b with DPM_F_BLEND); n, batch; sd / ed: state and network-output dtype; offset:
    elements every payload sits past its 16-byte boundary; dup: name x_out2 (duplicate store, or the corrected state with
    DPM_F_STORE_XC); stride: eps_stride in elements (0 = dense); blend = (mask_period, with blend_b); sep_xe: a separate
    evaluation state; ws_bytes: thresholding workspace (None: no workspace pointer); seed: of the
    data; noise_seed / per_request_stages: the launch options; resident: dpm_buffers.inputs_resident (the previous launch wrote
    the inputs).  `like`: another GuardedLaunch whose pristine payloads are copied (the same case on another device)."""

    def __init__(self, family, st, n, sd, ed, batch=1, device="cpu", offset=0, dup=False, stride=0, blend=None, sep_xe=False,
                 ws_bytes=None, seed=0, req=0, noise_seed=None, per_request_stages=False, like=None, coef64=None, resident=False):
        # coef64: the L.StageF64 of a double-precision plan (dpm_buffers.coef64), kept alive by the case; None: the record's
        # fp32 scalars, converted exactly
        self.coef64 = coef64 if coef64 is not None or like is None else getattr(like, "coef64", None)
        self.family, self.st, self.n, self.batch, self.sd, self.ed, self.req = family, st, int(n), int(batch), sd, ed, req
        self.offset, self.stride, self.blend, self.device = offset, int(stride), blend, device
        self.kw = dict(batch=batch, offset=offset, dup=dup, stride=stride, blend=blend, sep_xe=sep_xe, ws_bytes=ws_bytes, seed=seed,
                       req=req, noise_seed=noise_seed, per_request_stages=per_request_stages)
        self.resident = bool(resident or getattr(like, "resident", False))   # dpm_buffers.inputs_resident
        per = self.n // self.batch
        cfg = st.guidance == L.GUIDE["classifier-free"]
        unipc = st.form == L.FORM_UNIPC
        eps_extent = (self.batch - 1) * self.stride + per if self.stride else self.n
        want = {"x": (sd, self.n), "e0": (ed, eps_extent)}
        if sep_xe:
            want["xe"] = (sd, self.n)
        if cfg:
            want["e1"] = (ed, eps_extent)
        if st.guidance == L.GUIDE["classifier"]:
            want["g"] = (ed, self.n)
        if st.form in (L.FORM_TWO, L.FORM_MS3, L.FORM_SS3T) or unipc:
            want["h1"] = (sd, self.n)
        if st.form in (L.FORM_MS3, L.FORM_SS3T) or (unipc and st.flags & L.F_UNIPC_DP):
            want["h2"] = (sd, self.n)
        if st.flags & L.F_BLEND:
            want["mask"], want["blend_a"] = (sd, blend[0]), (sd, self.n)
            if blend[1]:
                want["blend_b"] = (sd, self.n)
        g = torch.Generator().manual_seed(1000003 * seed + req)
        self.arenas, self.pristine = {}, {}
        for k in INPUTS:
            if k not in want:
                continue
            dt, ext = want[k]
            if like is not None:
                bits = like.pristine[k]
            else:
                v = torch.rand(ext, generator=g) if k == "mask" else torch.randn(ext, generator=g)
                bits = v.to(dt).view(_INT[v.to(dt).element_size()])
            self.pristine[k] = bits
            self.arenas[k] = Arena(dt, ext, device, offset, bits=bits)
        for k in OUTPUTS:
            self.arenas[k] = Arena(sd, self.n, device, offset)
        self.arenas["workspace"] = Arena(torch.int32, (int(ws_bytes or 0) + 3) // 4, device, zero=True)
        self.named = {"x_out", "m_out"} | ({"x_out2"} if dup else set())      # the outputs the record points at
        self.written = {"x_out"} | ({"m_out"} if st.flags & L.F_STORE_M else set()) | ({"x_out2"} if dup else set())
        self.opts = L.LaunchOpts()
        self.opts.per_request_stages = 1 if per_request_stages else 0
        if noise_seed is not None:
            self.opts.noise_seed_lo, self.opts.noise_seed_hi = noise_seed & 0xFFFFFFFF, noise_seed >> 32
        self.b = self.buffers()

    def on(self, device):
        """the same case, pristine, on `device`"""
        return GuardedLaunch(self.family, self.st, self.n, self.sd, self.ed, device=device, like=self, coef64=self.coef64,
                             resident=self.resident, **self.kw)

    def buffers(self):
        b = L.Buffers()
        for k, a in self.arenas.items():
            if k in INPUTS or k in self.named or (k == "workspace" and self.kw["ws_bytes"] is not None):
                setattr(b, k, a.ptr)
        b.n, b.batch = self.n, self.batch
        b.state_dtype, b.eps_dtype = CODE[self.sd], CODE[self.ed]
        b.eps_stride = self.stride
        if self.blend is not None:
            b.mask_period = self.blend[0]
        b.opts = C.pointer(self.opts)
        if self.resident:
            b.inputs_resident = 1
        if self.coef64 is not None:
            b.coef64 = C.pointer(self.coef64)
        return b

    # -------------------------------------------------------------------------------------------
    def _fail(self, buffer, off, what):
        raise GuardError("family=%s pair=%s/%s n=%d request=%d buffer=%s offset=%d: %s" % (
            self.family, _name(self.sd), _name(self.ed), self.n, self.req, buffer, off, what))

    def verify(self, want=None, rc=0, noop=False):
        """the checks of the module docstring; `want`: the GuardedLaunch the double ran on (None: structure only); `noop`: the
        launch had to leave every arena alone although it returned 0 (a launch of a finished adaptive run)"""
        now = {k: a.raw.cpu() for k, a in self.arenas.items()}
        for k, a in self.arenas.items():                                          # 2 (and 6: outputs after an error)
            if k in INPUTS or rc != 0 or noop:
                d = now[k] != a.before
                if bool(d.any()):
                    self._fail(k, _first(d) - a.lead, "changed by a launch that %s" % (
                        "returned the error code %d" % rc if rc != 0 else "had to be a no-op" if noop else "may only read it"))
        if rc != 0 or noop:
            return
        for k in OUTPUTS + ("workspace",):
            a, v = self.arenas[k], now[k]
            fill = FILL[a.es]
            end = a.lead + a.extent
            for lo, hi in ((0, a.lead), (end, v.numel())):                        # 1
                d = v[lo:hi] != fill
                if bool(d.any()):
                    self._fail(k, lo + _first(d) - a.lead, "guard element overwritten")
            if k == "workspace":
                if bool((v[a.lead:end] != 0).any()):
                    self._fail(k, _first(v[a.lead:end] != 0), "workspace not left zero-filled")
                continue
            stale = v[a.lead:end] == fill
            if k not in self.written:                                             # 3
                if not bool(stale.all()):
                    self._fail(k, _first(~stale), "written by a stage that must not write it")
                continue
            if bool(stale.any()):                                                 # 4
                self._fail(k, _first(stale), "payload element still holds the fill pattern (not stored)")
            if want is None:
                continue
            wa = want.arenas[k]                                                   # 5
            wv = wa.raw.cpu()[wa.lead:wa.lead + wa.extent]
            if self.sd == torch.float64:
                g_, w_ = v[a.lead:end].view(torch.float64), wv.view(torch.float64)
                bound = F64_BOUND * float(w_.abs().max())
                d = ~((g_ - w_).abs() <= bound)
            else:
                d = v[a.lead:end] != wv
            if bool(d.any()):
                i = _first(d)
                self._fail(k, i, "value differs from the double: got bits %#x, want %#x" % (
                    int(v[a.lead + i]) & (2 ** (8 * a.es) - 1), int(wv[i]) & (2 ** (8 * a.es) - 1)))


def verify_all(devs, wants=None, rc=0):
    for r, d in enumerate(devs):
        d.verify(None if wants is None else wants[r], rc)


# ------------------------------------------------------------------------------------------------
# the doubles, through the arenas' raw pointers
# ------------------------------------------------------------------------------------------------
def double_launch(st, b):
    """the pointer-level numpy double of dpm_stage_launch for any stage this suite sweeps"""
    if st.flags & L.F_NOISE:
        return SD.launch_raw_noise_double(KD._Ref(st), KD._Ref(b), None)
    if st.form == L.FORM_UNIPC:
        return UD.launch_raw_double(KD._Ref(st), KD._Ref(b), None)
    return KD.launch_raw_double(KD._Ref(st), KD._Ref(b), None, allow_blend=True)


def run_double(case):
    """run the double on (CPU) `case`, check that it stayed inside its payloads, return the case"""
    assert double_launch(case.st, case.b) == 0
    case.verify()
    return case


def poke(ptr, values, es):
    """write integer bit patterns at a raw CPU address (the fake launchers of test_guarded_host.py)"""
    arr = np.asarray(values, dtype={2: np.int16, 4: np.int32, 8: np.int64}[es]).reshape(-1)
    C.memmove(ptr, arr.ctypes.data, arr.size * es)


def peek(ptr, count, es):
    out = np.empty(count, dtype={2: np.int16, 4: np.int32, 8: np.int64}[es])
    C.memmove(out.ctypes.data, ptr, count * es)
    return out
