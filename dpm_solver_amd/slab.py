"""Continuous batching of SMALL requests: a slab pool (`DPM_Solver.request_pool(slots=S)`).

`RequestPool` calls the network once per active request and advances 16 requests per stage launch; with hundreds of requests of
one or a few images each, a tick is hundreds of batch-1 network calls.  The slab pool turns the tick around:

    pool = dpm_solver.request_pool(slots=256)
    h = pool.submit(x_T, steps=20, order=2, condition=c)        # x_T of [b, *sample_shape] takes b of the 256 rows
    done = pool.step()                                          # {handle: result} of the requests that finished
    while pool:
        done.update(pool.step())

One row of the pool is one sample.  The pool owns two state slabs `[S, *sample_shape]` it ping-pongs between (`[2S, ...]` under
classifier-free guidance: a stage's duplicate store goes to row S + s, replacing torch.cat([x] * 2)), three history slabs for
the cached model values and, for a conditional network, a condition slab (`[2S, *cond_shape]` under guidance, the
unconditional half first).  A tick is

  * ONE network call on the whole current slab with a per-row time vector -- idle rows included, their output is ignored;
  * ONE host-to-device copy carrying the tick's table and the NEXT tick's time vector;
  * ONE stage kernel: dpm_stage_launch_multi in table mode (dpm_launch_opts.table_mode: DPM_TABLE_FILL on the host, the copy,
    DPM_TABLE_LAUNCH), every row a request of n = one sample with the stage record of its own position in its own plan.
    (Groups of 16 rows or fewer, and rows the fused kernels do not take, are launched as in a `RequestPool`, in the same call.)

The host side of a tick does not loop over requests: the stage records of every plan live in one numpy array, a tick gathers
them by (plan, position) and computes every pointer as base + row * stride.  Staging is a small ring of pinned buffers, each
guarded by the event behind its copy: no host synchronisation in steady state.  (A tick that admits requests pays a second,
small copy: the time vector that rode with the previous tick's table does not know them.)

Guarantee: every result is bit-identical to `sample(x, ...)` / `sample_unipc(x, ...)` on the request alone -- for a network
whose output row depends only on its input row, its time and its condition row.  A real network's own batch-variance (kernels
chosen by batch size, batch statistics) is outside this.  Occupancy below S wastes network work in proportion: every tick
evaluates all S rows; compaction of a sparse slab is out of scope.

Admitted: multistep ODE requests (`submit`) and UniPC requests (`submit_unipc`), unconditional or classifier-free (conditions
and the guidance scale may be per request: see "Per-request guidance" below).  Everything else is refused with NotImplementedError: see `submit`.

`request_pool(slots=S, sde=True)` also admits SDE-DPM-Solver++ requests: `submit(x, ..., sde=True, seed=...)`, with
`RequestPool.submit`'s checks and seed rules.  The tick's two calls then carry DPM_TABLE_NOISE: every SDE row is a row of the
table whatever their number -- one stage_kernel_table_noise launch beside the ODE / UniPC one -- with a noise record behind
the rows (the staging is sized for that section).  The noise contract indexes z over the REQUEST's flat [b, C, H, W] tensor
and a request's samples may sit in any rows, so sample k of a request travels with dpm_buffers.noise_sample0 = k: its row
starts the generator's counter at k * per_sample / 4 blocks.  Every SDE request keeps a dpm_launch_opts of its own (the
solver's + its seed) while it is active, and its rows point at it; row 0's options carry the call's flags and its own seed,
as in a `RequestPool`.  A tick is one network call, one copy and one launch per family present (ODE, UniPC + ODE, SDE).
An SDE pool refuses, at its first submit, a sample whose element count is not a multiple of 8 (its rows could not take the
table, and the counter base would have nowhere to go).
Guarantee: every SDE result is bit-identical to `sample_sde(x, seed=..., ...)` on the request alone, for any b, whichever
rows it landed in.  A pool built without `sde=True` refuses SDE requests and runs exactly as before.

`request_pool(slots=S, thresholding=True)` is the slab pool of a solver built with correcting_x0_fn="dynamic_thresholding"
(pixel-space models: many requests of one or a few 64x64 images).  A row is one sample, and a sample of at most 12288 elements
-- [3,64,64] exactly -- fits the LDS of one workgroup: the tick's two calls carry DPM_TABLE_THRESH, every thresholded row is a
row of the table whatever their number -- ONE stage_thresh_kernel_table launch, one workgroup per row, no cluster, no
workspace -- and a tick stays one network call, one copy and one launch.  Admitted: multistep ODE requests (`submit`),
unconditional or classifier-free, with per-request conditions; UniPC and SDE requests are refused by their own checks of a
thresholding solver.  At its first submit such a pool refuses a sample of more than 12288 elements, one whose element count
is no multiple of 8, and one whose row is no multiple of 16 bytes (the row could not take the table, and its lone launch
would need a workspace the pool does not hold).
Guarantee: every result is bit-identical to `sample(x, ...)` on the request alone, for any b, whichever rows it landed in.
Without `thresholding=True` a slab pool refuses a thresholding solver as before.

`request_pool(slots=S, inpaint=True)` also admits inpainting / DiffEdit requests: `submit(x, ..., blend=mb)`, `mb` a
`MaskBlend` that is a pure function of (stage, element) -- `x0=` with `noise=` given (the fixed-noise re-noising of the known
image), or `intermediates=` (DiffEdit); `time_fn` is honoured, evaluated once per stage of the plan at submit.  The tick's two
calls then carry DPM_TABLE_BLEND: every blend row is a row of the table whatever their number -- one
stage_kernel_table_blend launch beside the plain family's -- with a blend record behind the rows (and behind the noise
records of an `sde=True` pool; the staging is sized for that section).  Admission materialises, once per request, in the state
dtype and contiguous: the mask at its own period (a `[H,W]` mask stays H*W elements; a period that is no multiple of 8 is
expanded to the full sample), the known image, the noise, one tensor per step for `intermediates`, and per-stage arrays of
(alpha, sigma) from the host schedule; the pool keeps them alive while the request is active or waiting.  A steady tick stays
vectorised: DPM_F_BLEND is or-ed into the flags of every blend row's record, blend_alpha / blend_sigma and the three
pointers are gathered by (request, position) and computed as base + sample * stride, mask_period is per row.  On the tick
that admits such a request its rows of the current state slab are blended after the network call and before the stage launch,
as `sample()` blends x_T after the first evaluation (dpm_blend_launch through a temporary -- the kernel's operands are
__restrict__ --, once per run of consecutive rows; both halves under guidance): launches on admitting ticks only.  A row
the table kernel does not take (the DENOISE stage of denoise_to_zero) goes as its own launch in the same call, which blends.
Guarantee: the result is bit-identical to `sample(x, ...)` of a solver built with `correcting_xt_fn=mb` on the request alone,
for any b, whichever rows it landed in.  Refused with NotImplementedError: `blend=` in a pool built without `inpaint=True`;
`MaskBlend(x0=..., noise=None)` (it draws torch.randn per call: pass `noise=`); `blend=` with `sde=True` (the table has no
blend behind the noise epilogue); `inpaint=True` with `thresholding=True` (the thresholded rows have no blend); `submit_unipc`
takes no blend.  Without `inpaint=True` every pool behaves and refuses as before.

`request_pool(slots=S, rescale=True)` is the slab pool that admits guidance-rescale requests (`dpm_solver_amd.cfg_rescale`;
v-prediction / zero-terminal-SNR checkpoints at the usual guidance scales): an effectively classifier-free wrapper, with or
without a phi of its own.  The tick's two calls carry DPM_TABLE_RESCALE: every row whose record carries DPM_F_CFG_RESCALE is a
row of the table whatever their number -- ONE stage_rescale_kernel_table launch, one workgroup per row, the kernel of the
request's own launch -- beside the plain family's, which rows with phi 0 take; a tick stays one network call, one copy and one
launch per family present.  A rescale row is a row and nothing else: no record section.  The DENOISE stage of
denoise_to_zero is a rescale row too.  At its first submit such a pool refuses a sample of fewer than 8 elements, one whose
element count is no multiple of 8, and one whose row is no multiple of 16 bytes (the row could not take the table).  Refused
with NotImplementedError: `rescale=True` with `sde=True`, `thresholding=True` or `inpaint=True` (the rescale kernel has none of
those epilogues); `submit_unipc` on a solver whose wrapper carries phi.  Without `rescale=True` a slab pool refuses a
`cfg_rescale` solver as before.

Per-request guidance: the kernels read the guidance scale and phi from each row's own record and no grouping key compares
them, so in ANY classifier-free slab pool `submit(..., guidance_scale=g)` / `submit_unipc(..., guidance_scale=g)` take the
request's own scale, and in a `rescale=True` pool `submit(..., guidance_rescale=phi)` its own phi in [0, 1]; the default for
both is the wrapper's.  The values are kept per row; every tick writes them over the gathered stage records, vectorised like
the blend fields, as the planner and the binder write them for a wrapper of that scale and phi (`_device._cfg_fields`): fp32(g)
in cfg_scale, DPM_F_CFG_RESCALE and phi in cg_scale -- phi 0 clears the flag: a plain row.  `guidance_scale=1.0` is refused
(NotImplementedError): a wrapper of scale 1 evaluates the conditional branch alone, without a blend, which a row of a
[2S, ...] slab cannot reproduce.  Either argument on a pool whose wrapper is not classifier-free, a g that is no real number
and a phi outside [0, 1] are ValueError; `guidance_rescale=` outside a `rescale=True` pool is NotImplementedError.
Guarantee: every result is bit-identical to `sample(x, ...)` on the request alone, on a solver whose wrapper has the request's
guidance scale and `cfg_rescale(..., phi)`, for any b, whichever rows it landed in.

`request_pool(slots=S, apg=True)` is the slab pool that admits adaptive-projected-guidance requests
(`dpm_solver_amd.cfg_apg`): an effectively classifier-free wrapper on a data-prediction solver, with or without APG parameters
of its own.  The tick's two calls carry DPM_TABLE_APG: every row whose record carries DPM_F_CFG_APG is a row of the table
whatever their number -- ONE stage_apg_kernel_table launch, one workgroup per row, the kernel of the request's own launch --
beside the plain family's, which rows of parameters (1, 0, 0) take; behind the rows the table has an APG record per row (the
staging is sized for that section).  What APG has and no other kind has is state that persists per request: with a momentum a
request carries an fp32 running average of the guidance direction from evaluation to evaluation.  The pool holds the averages
in one fp32 slab `[S, *sample_shape]`, allocated with the other slabs; in a DPM_TABLE_APG call a request's average is
dpm_buffers.thr_hint (bs[0].workspace is the table), so every tick writes thr_hint = slab + row * per_sample * 4 into the
buffer records of the rows whose record has a momentum and 0 into the others, vectorised.  Admission zero-fills the rows it
takes -- one zero_() per run of consecutive rows, on admitting ticks only, before the tick's launch: a request starts from a
zero average whatever request used its rows before.  The DENOISE stage of denoise_to_zero is an APG row too and updates the
average, as in `sample()`.  Per request: `submit(..., apg=(eta, norm_threshold, momentum))`, checked with `cfg_apg`'s ranges and
texts; the default is the wrapper's.  The values are kept per row; every tick writes them over the gathered records as
`_bind_apg` writes them for a wrapper of those parameters (`_device._apg_fields`): DPM_F_CFG_APG, eta in cg_scale, the norm
threshold in thr_ratio, the momentum in thr_max -- (1.0, 0.0, 0.0) clears the flag and restores the plain classifier-free
fields: a plain row, as `cfg_apg(fn, 1, 0, 0)` is plain.  `guidance_scale=` works as in every classifier-free pool.  At its
first submit such a pool refuses a sample of fewer than 8 elements, one whose element count is no multiple of 8, and one whose
row is no multiple of 16 bytes.  Refused with NotImplementedError: `apg=True` with `rescale=True`, `sde=True`,
`thresholding=True` or `inpaint=True` (the APG kernel has none of those epilogues); `submit_unipc` on a solver whose wrapper
carries APG parameters; `apg=` outside an `apg=True` pool.  `apg=` on a pool whose wrapper is not classifier-free is
ValueError.  Without `apg=True` a slab pool refuses a `cfg_apg` solver as before.
Guarantee: every result is bit-identical to `sample(x, ...)` on the request alone, on a solver whose wrapper has the request's
guidance scale and `cfg_apg(fn, *its parameters)`, for any b, whichever rows it landed in and whatever request used those rows
before.

`request_pool(slots=S, zero_star=True)` is the slab pool that admits CFG-Zero* requests (`dpm_solver_amd.cfg_zero_star`): an
effectively classifier-free wrapper, with or without the setting of its own.  The tick's two calls carry DPM_TABLE_ZSTAR: every
row whose record carries DPM_F_CFG_ZSTAR is a row of the table whatever their number -- ONE stage_zstar_kernel_table launch, one
workgroup per row, the kernel of the request's own launch -- beside the plain family's, which rows without the flag take; a
tick stays one network call, one copy and one launch per family present.  A CFG-Zero* row is a row and nothing else: the kind
has no parameter and no state, so there is no record section and nothing to reset at admission.  The DENOISE stage of
denoise_to_zero is a CFG-Zero* row too.  Per request: `submit(..., zero_star=True | False)`; the default is the wrapper's.  The
choice is kept per row; every tick writes it over the gathered records as `_bind_zstar` writes it: DPM_F_CFG_ZSTAR set or
cleared on classifier-free rows -- cleared: a plain row.  `guidance_scale=` works as in every classifier-free pool.  At its
first submit such a pool refuses a sample of fewer than 8 elements, one whose element count is no multiple of 8, and one whose
row is no multiple of 16 bytes (the row could not take the table).  Refused with NotImplementedError: `zero_star=True` with
`rescale=True`, `apg=True`, `sde=True`, `thresholding=True` or `inpaint=True` (the CFG-Zero* kernel has none of those
epilogues); `submit_unipc` on a solver whose wrapper carries the setting; `zero_star=True` outside a `zero_star=True` pool.
`zero_star=` on a pool whose wrapper is not classifier-free, and a value that is no bool, are ValueError.  Without
`zero_star=True` a slab pool refuses a `cfg_zero_star` solver as before.
Guarantee: every result is bit-identical to `sample(x, ...)` on the request alone, on a solver whose wrapper has the request's
guidance scale and `cfg_zero_star` (or not), for any b, whichever rows it landed in.

`request_pool(slots=S, pair=True)` is the slab pool of a `dpm_solver_amd.cfg_pair` wrapper: guidance over two conditions
(InstructPix2Pix's image and text scales, composable conditions).  The network's input is THREE copies of every state, so the
state slabs are [3S, ...], the time vector has 3S entries and the condition slab is [3S, *cond_shape] in the wrapper's order --
unconditional, condition, condition2 --: the one network call's output chunks as `e1, e0, e2 = out.chunk(3)`, exactly as
`WrappedModel.raw_outputs` chunks it.  Admission writes x_T into all three thirds.  The tick's two calls carry DPM_TABLE_PAIR:
every row is a DPM_GUIDE_CFG2 row of the table -- ONE stage_pair_kernel_table launch, the arithmetic of the request's own
stage_pair_kernel launch -- with a pair record behind it: g = e2 + row, and the THIRD copy of x_out in dpm_buffers.thr_hint
(x_out2 = xout + (S + row), thr_hint = xout + (2S + row); both zero on a request's last stage).  The kernel stores the result
three times, so no tick runs a `torch.cat([x] * 3)`; a tick stays one network call, one copy and one launch.  The DENOISE stage
of denoise_to_zero is a row too.  Per request: `submit(..., condition=, unconditional_condition=, condition2=,
guidance_scale=s, pair=(scale2, nested))` -- s1 = fp32(s), s2 = scale2, or scale2 - s under nested=True, formed in double and
rounded once: exactly `cfg_pair` and `_prep_stage`, with cfg_pair's range checks and texts.  Both scales are kept per row;
every tick writes them over the gathered records (cfg_scale, cg_scale).  The defaults are the wrapper's own values.
`guidance_scale=` without `pair=` is ValueError (the wrapper does not keep `nested`, so the second scale's meaning would be a
guess); `guidance_scale=1.0` is fine here: a pair wrapper always evaluates three branches.  A request whose s2 comes out 0 is
NotImplementedError: it would be plain two-branch guidance, which for half noise networks blends in half, and a row of a [3S]
slab cannot reproduce those bits.  At its first submit such a pool refuses a sample of fewer than 8 elements, one whose
element count is no multiple of 8, and one whose row is no multiple of 16 bytes.  Refused with NotImplementedError:
`pair=True` with `sde`, `thresholding`, `inpaint`, `rescale`, `apg` or `zero_star`; `submit_unipc`; `submit(sde=True)`;
`blend=`; `pair=` outside a `pair=True` pool.  `pair=True` on a solver whose wrapper is no `cfg_pair` one, and without
`slots`, are ValueError.  Without `pair=True` a pool refuses a `cfg_pair` solver as before.
Guarantee: every result is bit-identical to `sample(x, ...)` on the request alone, on a solver whose wrapper is
`cfg_pair(model_wrapper(..., guidance_scale=s, condition=c, unconditional_condition=u), c2, scale2, nested)`, for any b,
whichever rows it landed in.

`request_pool(slots=S, perp_neg=True)` is the slab pool of a `dpm_solver_amd.cfg_perp_neg` wrapper: Perp-Neg guidance, the
negative prompt's direction taken perpendicular to the positive one's, per image.  Everything about the slabs is the pair pool's:
state slabs of [3S, ...], a time vector of 3S entries, a condition slab [3S, *cond_shape] in the wrapper's order -- empty
prompt, positive, negative --, the one network call's output chunked as `e1, e0, e2 = out.chunk(3)`, exactly as
`WrappedModel.raw_outputs` chunks it, x_T written into all three thirds at admission.  The tick's two calls carry
DPM_TABLE_PERP: every row is a Perp-Neg row of the table -- ONE stage_perp_kernel_table launch per group, one workgroup per
sample running the source of the request's own stage_perp_kernel launch -- with a pair record behind it: g = e2 + row, and the
THIRD copy of x_out in dpm_buffers.thr_hint (x_out2 = xout + (S + row), thr_hint = xout + (2S + row); both zero on a request's
last stage).  The kernel stores the result three times, so no tick runs a `torch.cat([x] * 3)`; a tick stays one network call,
one copy and one launch per group.  The DENOISE stage of denoise_to_zero is a row too.  Per request: `submit(..., condition=,
unconditional_condition=, negative_condition=, guidance_scale=s, neg_scale=w)` -- either scale without the other: they are
independent, unlike cfg_pair's `nested` --, checked as `cfg_perp_neg` checks them, with its texts.  Both scales are kept per row;
every tick writes them over the gathered records (cfg_scale = s, cg_scale = w); the flag stays as `_prep_stage` bound it.  The
defaults are the wrapper's own values.  A request with w == 0 is NotImplementedError: it would be plain two-branch guidance,
which for half noise networks blends in half, and a row of a [3S] slab cannot reproduce those bits.  At its first submit such a
pool refuses a sample of fewer than 8 elements, one whose element count is no multiple of 8, and one whose row is no multiple
of 16 bytes.  Refused with NotImplementedError: `perp_neg=True` with `sde`, `thresholding`, `inpaint`, `rescale`, `apg`,
`zero_star` or `pair`; `submit_unipc`; `submit(sde=True)`; `blend=`; `negative_condition=` / `neg_scale=` outside a
`perp_neg=True` pool; `condition2=` / `pair=` inside one.  `perp_neg=True` on a solver whose wrapper is no `cfg_perp_neg` one
(a plain `cfg_pair` wrapper included), and without `slots`, are ValueError.  Without `perp_neg=True` a slab pool refuses a
`cfg_perp_neg` solver as before (`pair=True` with its own text).
Guarantee: every result is bit-identical to `sample(x, ...)` on the request alone, on a solver whose wrapper is
`cfg_perp_neg(model_wrapper(..., guidance_scale=s, condition=c, unconditional_condition=u), n, w)`, for any b, whichever rows
it landed in and whoever used them before.
"""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _device as DV
from . import _lib as L
from . import remedies as _rem
from . import sde as _sde
from . import unipc as _unipc
from .correctors import MaskBlend
from .wrapper import apg_params

_RING = 4
_STAGE = np.dtype(L.Stage)
# an inpainting request's blend at one position of its plan: DPM_F_BLEND or 0, the scalars, the known image / noise of sample 0
_BLEND = np.dtype([("flag", np.uint32), ("alpha", np.float32), ("sigma", np.float32), ("a", np.uint64), ("b", np.uint64)])
_BUFS = np.dtype(dict(names=[{"_ns0": "noise_sample0"}.get(n, n) for n, _ in L.Buffers._fields_],
                      formats=[{4: np.int32, 8: np.uint64}[getattr(L.Buffers, n).size] for n, _ in L.Buffers._fields_],
                      offsets=[getattr(L.Buffers, n).offset for n, _ in L.Buffers._fields_], itemsize=C.sizeof(L.Buffers)))
assert _STAGE.itemsize == C.sizeof(L.Stage)

# What a row holds: (name, numpy dtype, idle value).  The pool keeps one array `_<name>` of S entries per field, and admission
# resets EVERY field of the rows it takes to the idle value before it writes the request's own: a row that passes from a
# request of one kind to a request of another carries nothing over, and a field added here cannot forget its reset.
_ROW = (
    ("req", np.int64, -1),       # its request's handle (-1: idle)
    ("off", np.int64, 0),        # its plan's offset into the record array
    ("pos", np.int64, 0),        # its position in its plan
    ("len", np.int64, 0),        # its plan's length
    ("samp", np.int32, 0),       # the sample of its request it holds: request rows[k] holds sample k
    # SDE rows (see "SDE requests" below)
    ("optp", np.uint64, 0),      # its request's dpm_launch_opts (0: the solver's)
    ("seed", np.uint64, 0),      # its request's seed
    # per-request guidance (see "per-request guidance" below)
    ("gon", np.bool_, False),    # does its request bring its own guidance (submit's guidance_scale= / guidance_rescale=)?
    ("gs", np.float32, 0),       # its guidance scale
    ("gphi", np.float32, 0),     # its phi
    # adaptive projected guidance (see "adaptive projected guidance" below)
    ("aon", np.bool_, False),    # does its request bring its own APG parameters (submit's apg=)?
    ("aeta", np.float32, 1),     # its eta, norm threshold and momentum; (1, 0, 0): classifier-free guidance itself
    ("ar", np.float32, 0),
    ("abeta", np.float32, 0),
    # CFG-Zero* (see "CFG-Zero*" below)
    ("zon", np.bool_, False),    # does its request bring its own choice (submit's zero_star=)?
    ("zsel", np.bool_, False),   # its choice: the CFG-Zero* projection, or plain classifier-free guidance
    # guidance over two conditions (see "guidance over two conditions" below)
    ("ps1", np.float32, 0),      # its two scales: cfg_scale and cg_scale of its DPM_GUIDE_CFG2 records
    ("ps2", np.float32, 0),
    # inpainting rows (see "inpainting requests" below)
    ("bslot", np.int64, -1),     # the first row of its inpainting request: where _brec holds its blend records (-1: none)
    ("bmask", np.uint64, 0),     # the mask of its sample
    ("bper", np.int64, 0),       # its mask period
)

# The first-submit check of a sample's element count, per kind the pool was built with, in this order: (the pool's switch, the
# smallest and the largest admissible count, the message).  Every kind wants whole 8-element groups of 16-byte aligned rows.
_GROUPS = "whole 8-element groups of 16-byte aligned buffers; use request_pool() without slots"
_ROW_CHECKS = (
    ("_sde", 0, math.inf, "slab pool: sde=True with a sample of %d elements -- a row of the table noise kernel is " + _GROUPS),
    ("_rsc", 8, math.inf, "slab pool: rescale=True with a sample of %d elements -- a rescale row of the table is " + _GROUPS),
    ("_apg", 8, math.inf, "slab pool: apg=True with a sample of %d elements -- an APG row of the table is " + _GROUPS),
    ("_zst", 8, math.inf, "slab pool: zero_star=True with a sample of %d elements -- a CFG-Zero* row of the table is " + _GROUPS),
    ("_pr", 8, math.inf, "slab pool: pair=True with a sample of %d elements -- a two-condition row of the table is " + _GROUPS),
    ("_pn", 8, math.inf, "slab pool: perp_neg=True with a sample of %d elements -- a Perp-Neg row of the table is " + _GROUPS),
    ("_thr", 0, L.THR_ROW_MAX, "slab pool: thresholding=True with a sample of %%d elements -- a thresholded row of the table is "
                               "at most %d elements (one workgroup's LDS), " % L.THR_ROW_MAX + _GROUPS),
)


def _esize(dtype):
    """bytes per element of a torch dtype"""
    return torch.empty((), dtype=dtype).element_size()


def _runs(rows):
    """the sorted row list as (first, count) runs of consecutive rows"""
    out = []
    for r in rows:
        if out and out[-1][0] + out[-1][1] == r:
            out[-1][1] += 1
        else:
            out.append([r, 1])
    return out


class _Waiting:
    __slots__ = ("h", "x", "plan", "cond", "uncond", "mf", "seed", "blend", "guide", "apg", "zstar", "cond2", "pair")


class _Blend:
    """what an inpainting request keeps alive: its tensors, its per-stage records, and the blend of x_T (`first`)"""
    __slots__ = ("keep", "rec", "mask", "mstep", "period", "first")


class _Slot:
    """one slot of the staging ring: the pinned buffer, the device buffers for its first two parts (`dev`) and for the third
    (`devt`), the event behind its table copy, and views of the pinned parts (`pin_cur`: this tick's times as a tensor)"""
    __slots__ = ("pin", "dev", "devt", "ev", "t_next", "t_cur", "st", "bufs", "bufs_raw", "pin_cur")


class SlabPool:
    """`slots` rows of one sample shape, dtype and device (fixed by the first submit); see the module docstring."""

    def __init__(self, solver, slots, sde=False, thresholding=False, inpaint=False, rescale=False, apg=False,
                 zero_star=False, pair=False, perp_neg=False):
        slots = int(slots)
        if slots < 1:
            raise ValueError("request_pool: slots must be a positive number of rows, got %d" % slots)
        self._s, self.S = solver, slots
        self._sde = bool(sde)            # SDE requests admitted: the tick's calls carry DPM_TABLE_NOISE
        self._thr = bool(thresholding)   # a thresholding solver's pool: the tick's calls carry DPM_TABLE_THRESH
        self._inp = bool(inpaint)        # inpainting requests admitted: the tick's calls carry DPM_TABLE_BLEND
        self._rsc = bool(rescale)        # guidance-rescale requests admitted: the tick's calls carry DPM_TABLE_RESCALE
        self._apg = bool(apg)            # adaptive-projected-guidance requests admitted: the tick's calls carry DPM_TABLE_APG
        self._zst = bool(zero_star)      # CFG-Zero* requests admitted: the tick's calls carry DPM_TABLE_ZSTAR
        self._pr = bool(pair)            # a cfg_pair solver's pool, slabs of [3S, ...]: the tick's calls carry DPM_TABLE_PAIR
        self._pn = bool(perp_neg)        # a cfg_perp_neg solver's pool, slabs of [3S, ...]: the tick's calls carry DPM_TABLE_PERP
        self._three = self._pr or self._pn   # three network outputs per row: the third condition in q.cond2, the scales in q.pair
        self._tflags = ((L.TABLE_NOISE if self._sde else 0) | (L.TABLE_THRESH if self._thr else 0)
                        | (L.TABLE_BLEND if self._inp else 0)       # ... the flags of every tick's two calls, and its table's size
                        | (L.TABLE_RESCALE if self._rsc else 0) | (L.TABLE_APG if self._apg else 0)
                        | (L.TABLE_ZSTAR if self._zst else 0) | (L.TABLE_PAIR if self._pr else 0)
                        | (L.TABLE_PERP if self._pn else 0))
        self._avg = None                 # (an apg=True pool) the running averages: one fp32 slab [S, *sample_shape]
        self._cols = []                  # the per-row arrays of _ROW (self._req, self._pos, ...), each with its idle value
        for name, dtype, idle in _ROW:
            setattr(self, "_" + name, np.full(slots, idle, dtype=dtype))
            self._cols.append((getattr(self, "_" + name), idle))
        self._blends = {}                # handle -> the _Blend of an active inpainting request
        self._brec = np.zeros((slots, 0), dtype=_BLEND)  # [first row of the request, position]: its blend records
        self._ropts = {}                 # handle -> the dpm_launch_opts of an active SDE request (the solver's + its seed)
        self._wait = []                  # FIFO of _Waiting: requests that found too few free rows
        self._rows = {}                  # handle -> (rows, memory format of x_T) of the admitted requests
        self._free = list(range(slots))  # sorted
        self._next = 0
        self._like = None                # (sample shape, dtype, device)
        self._plans = {}                 # id(plan) -> (offset into the record arrays, plan)
        self._recs = np.zeros(0, dtype=_STAGE)
        self._opts = L.LaunchOpts()
        self._tick = 0
        self._t_next = None              # host copy of the time vector that rode with the last table, and where it is
        self._t_dev = None
        self.copies = 0                  # host-to-device copies issued (diagnostics: one per tick in steady state)

    def __len__(self):
        return len(self._rows) + len(self._wait)

    def __bool__(self):
        return len(self) > 0

    # ------------------------------------------------------------------------------------------------------------------
    # submitting
    # ------------------------------------------------------------------------------------------------------------------
    def _refuse(self, method='multistep', sde=False, return_intermediate=False):
        s = self._s
        if method != 'multistep':
            raise NotImplementedError("slab pool: method={!r} -- a singlestep or adaptive update evaluates the network on an "
                                      "intermediate state, and a slab row's evaluation state is its state; use "
                                      "request_pool() without slots".format(method))
        if sde and not self._sde:
            raise NotImplementedError("slab pool: sde=True -- SDE stages have no table kernel; use request_pool() without slots")
        if s._thresholding and not self._thr:
            raise NotImplementedError("slab pool: correcting_x0_fn='dynamic_thresholding' -- thresholded stages have no table "
                                      "kernel; use request_pool() without slots")
        if s._wrapped is not None and s._wrapped.effective_guidance == "classifier":
            raise NotImplementedError("slab pool: classifier guidance -- the classifier's gradient is a second network call per "
                                      "request; use request_pool() without slots")
        if s._user_x0 is not None or s.correcting_xt_fn is not None:
            raise NotImplementedError("slab pool: a correcting_x0_fn / correcting_xt_fn runs Python between stages; sample with "
                                      "sample()")
        if return_intermediate:
            raise NotImplementedError("slab pool: return_intermediate is not supported; sample it with sample()")
        _rem.check_slab(s, {"rescale": self._rsc, "apg": self._apg, "zero_star": self._zst})

    def _apg_params(self, apg):
        """the request's own (eta, norm threshold, momentum) of submit's apg=, checked as cfg_apg checks them; None: the
        wrapper's"""
        if apg is None:
            return None
        w = self._s._wrapped
        if w is None or w.effective_guidance != "classifier-free":
            raise ValueError("slab pool: apg= belongs to a classifier-free wrapper (with an unconditional condition and a "
                             "guidance scale other than 1)")
        if not isinstance(apg, (tuple, list)) or len(apg) != 3:
            raise ValueError("slab pool: apg= takes (eta, norm_threshold, momentum), got %r" % (apg,))
        apg = apg_params(*apg)
        if not self._apg:
            raise NotImplementedError("slab pool: apg= -- projected-guidance stages take the table in a pool built with "
                                      "request_pool(slots=..., apg=True) only")
        return apg

    def _zstar_choice(self, on):
        """the request's own choice of submit's zero_star=, checked; None: the wrapper's"""
        if on is None:
            return None
        w = self._s._wrapped
        if w is None or w.effective_guidance != "classifier-free":
            raise ValueError("slab pool: zero_star= belongs to a classifier-free wrapper (with an unconditional condition and a "
                             "guidance scale other than 1)")
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("slab pool: zero_star= takes True or False, got %r" % (on,))
        if on and not self._zst:
            raise NotImplementedError("slab pool: zero_star= -- CFG-Zero* stages take the table in a pool built with "
                                      "request_pool(slots=..., zero_star=True) only")
        return bool(on)

    def _perp_params(self, scale, neg_scale, neg_cond, pair, cond2):
        """the request's own (s, w) of submit's guidance_scale= / neg_scale=, checked as cfg_perp_neg checks them; None: the
        wrapper's"""
        if not self._pn:
            if neg_scale is not None or neg_cond is not None:
                raise NotImplementedError("slab pool: %s= -- Perp-Neg stages take the table in a pool built with "
                                          "request_pool(slots=..., perp_neg=True) only"
                                          % ("neg_scale" if neg_scale is not None else "negative_condition"))
            return None
        if pair is not None or cond2 is not None:
            raise NotImplementedError("slab pool: %s= in a perp_neg=True pool -- the Perp-Neg kernel takes one negative "
                                      "condition (negative_condition=, neg_scale=) and no second blend"
                                      % ("pair" if pair is not None else "condition2"))
        if scale is None and neg_scale is None:
            return None
        s0, w0 = self._s._pair_setting()
        w = w0 if neg_scale is None else neg_scale
        if isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(float(w)):
            raise ValueError("cfg_perp_neg: neg_scale must be a finite real number, got %r" % (w,))
        sc = s0 if scale is None else scale
        if isinstance(sc, bool) or not isinstance(sc, numbers.Real) or not math.isfinite(float(sc)):
            raise ValueError("cfg_perp_neg: the wrapper's guidance_scale must be a finite real number, got %r" % (sc,))
        if float(w) == 0.0:
            raise NotImplementedError("slab pool: neg_scale=%r -- a negative scale of 0 is plain two-branch guidance: for half "
                                      "noise networks that blends in half, and a row of a [3S] slab cannot reproduce those bits"
                                      % (w,))
        return float(sc), float(w)

    def _pair_params(self, scale, pair, cond2):
        """the request's own (s1, s2) of submit's guidance_scale= / pair=, checked as cfg_pair checks them; None: the wrapper's"""
        if self._pn:
            return None                  # (a perp_neg=True pool: _perp_params has spoken)
        if not self._pr:
            if pair is not None:
                raise NotImplementedError("slab pool: pair= -- two-condition stages take the table in a pool built with "
                                          "request_pool(slots=..., pair=True) only")
            if cond2 is not None:
                raise ValueError("slab pool: condition2= belongs to a pool built with request_pool(slots=..., pair=True)")
            return None
        if pair is None:
            if scale is not None:
                raise ValueError("slab pool: guidance_scale= in a pair=True pool needs pair=(scale2, nested) -- the wrapper does "
                                 "not keep `nested`, so the second scale's meaning would be a guess")
            return None
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("slab pool: pair= takes (scale2, nested), got %r" % (pair,))
        scale2, nested = pair
        if isinstance(scale2, bool) or not isinstance(scale2, numbers.Real) or not math.isfinite(float(scale2)):
            raise ValueError("cfg_pair: scale2 must be a finite real number, got %r" % (scale2,))
        if not isinstance(nested, (bool, np.bool_)):
            raise ValueError("cfg_pair: nested must be a bool, got %r" % (nested,))
        sc = self._s._wrapped.guidance_scale if scale is None else scale
        if isinstance(sc, bool) or not isinstance(sc, numbers.Real) or not math.isfinite(float(sc)):
            raise ValueError("cfg_pair: the wrapper's guidance_scale must be a finite real number, got %r" % (sc,))
        s1, s2 = float(sc), (float(scale2) - float(sc) if nested else float(scale2))
        if s2 == 0.0:
            raise NotImplementedError("slab pool: pair=%r with guidance_scale=%r -- the second scale comes out 0, which is plain "
                                      "two-branch guidance: for half noise networks that blends in half, and a row of a [3S] "
                                      "slab cannot reproduce those bits" % (tuple(pair), sc))
        return s1, s2

    def _guidance(self, scale, phi):
        """the request's own (guidance scale, phi) of submit's guidance_scale= / guidance_rescale=, checked; None: the wrapper's"""
        if scale is None and phi is None:
            return None
        w = self._s._wrapped
        if w is None or w.effective_guidance != "classifier-free":
            raise ValueError("slab pool: guidance_scale / guidance_rescale belong to a classifier-free wrapper (with an "
                             "unconditional condition and a guidance scale other than 1)")
        for name, v in (("guidance_scale", scale), ("guidance_rescale", phi)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Real) or not np.isfinite(float(v))):
                raise ValueError("slab pool: %s must be a real number, got %r" % (name, v))
        if phi is not None and not (0.0 <= float(phi) <= 1.0):
            raise ValueError("slab pool: guidance_rescale must be in [0, 1], got %r" % (phi,))
        if scale is not None and float(scale) == 1.0:
            raise NotImplementedError("slab pool: guidance_scale=1.0 -- a wrapper of scale 1 evaluates the conditional branch "
                                      "alone, without a blend, which a row of a classifier-free slab cannot reproduce")
        if phi is not None and not self._rsc:
            raise NotImplementedError("slab pool: guidance_rescale= -- rescale stages take the table in a pool built with "
                                      "request_pool(slots=..., rescale=True) only")
        return (float(w.guidance_scale) if scale is None else float(scale),
                float(self._s._remedy_setting("cfg_rescale") or 0.0) if phi is None else float(phi))

    def _check_state(self, x):
        """the refusals that depend on x's dtype, then the device requirement and the pool's own checks"""
        s = self._s
        sd = s._sdtype(x)
        if sd is torch.float64:
            raise NotImplementedError("slab pool: double-precision states (the table kernels take 2- and 4-byte states)")
        if sd in (torch.float16, torch.bfloat16) and s._state_dtype is None:
            raise NotImplementedError("slab pool: a half-precision slab needs a solver built with an explicit state_dtype -- "
                                      "the reference's type promotion would depend on the first network output")
        if self._like is None and torch.is_tensor(x) and x.dim() >= 1 and x.numel() > 0:
            per = x.numel() // x.shape[0]
            for switch, lo, hi, text in _ROW_CHECKS:
                if getattr(self, switch) and not (lo <= per <= hi and per % 8 == 0 and (per * _esize(sd)) % 16 == 0):
                    raise NotImplementedError(text % per)
        DV._require_gpu(x)
        if not torch.is_tensor(x) or x.dim() < 1 or x.numel() == 0:
            raise ValueError("slab pool: x must be a tensor [b, *sample_shape] with at least one element")
        like = (tuple(x.shape[1:]), x.dtype, x.device)
        if self._like is not None and like != self._like:
            raise ValueError("slab pool: x of sample shape %s, dtype %s on %s does not match the pool's %s, %s on %s"
                             % (like + self._like))
        if x.shape[0] > self.S:
            raise ValueError("slab pool: a request of %d samples does not fit %d slots" % (x.shape[0], self.S))
        return like, sd

    def submit(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', method='multistep',
               lower_order_final=True, denoise_to_zero=False, solver_type='dpmsolver', return_intermediate=False, sde=False,
               condition=None, unconditional_condition=None, seed=None, generator=None, blend=None, guidance_scale=None,
               guidance_rescale=None, apg=None, zero_star=None, condition2=None, pair=None, negative_condition=None,
               neg_scale=None):
        """Admit a multistep ODE request: `x` = its x_T of [b, *sample_shape] (b rows, any rows), the rest as for `sample()`,
        validated with sample()'s errors in its order before any device work.  `condition` / `unconditional_condition`: the
        request's own, of leading dimension b or 1 (default: the wrapper's).  Refused with NotImplementedError: singlestep and
        adaptive methods, sde=True in a pool built without it, a thresholding solver in a pool built without thresholding=True, classifier guidance, correcting_x0_fn / correcting_xt_fn,
        return_intermediate, double states, and a half-precision slab on a solver without an explicit state_dtype.  A request
        that finds fewer than b free rows waits (first in, first out) and is admitted by a later step().  Returns the
        request's handle.
        `sde=True` (a pool built with sde=True): an SDE-DPM-Solver++ request -- `sample_sde`'s arguments, checks and seed rules
        (`seed`, or one draw from `generator` / torch's default CPU generator, made here), as `RequestPool.submit`.
        `blend=mb` (a pool built with inpaint=True): an inpainting / DiffEdit request -- the result of `sample()` on a solver
        built with correcting_xt_fn=mb; see the module docstring for the forms of `MaskBlend` admitted.
        `guidance_scale=g` (a classifier-free pool): the request's own guidance scale -- the result of `sample()` on a solver
        whose wrapper has that scale; g = 1.0 is refused.  `guidance_rescale=phi` (a pool built with rescale=True): the request's
        own phi in [0, 1] -- the result of `sample()` under `cfg_rescale(model_fn, phi)`.  Default for both: the wrapper's.
        `apg=(eta, norm_threshold, momentum)` (a pool built with apg=True): the request's own adaptive projected guidance --
        the result of `sample()` under `cfg_apg(model_fn, eta, norm_threshold, momentum)`; (1.0, 0.0, 0.0) is classifier-free
        guidance itself.  Default: the wrapper's.
        `zero_star=True | False` (True: a pool built with zero_star=True): the request's own choice of the CFG-Zero*
        projection -- the result of `sample()` under `cfg_zero_star(model_fn)`, or under the bare wrapper.  Default: the
        wrapper's.
        `condition2=c2, guidance_scale=s, pair=(scale2, nested)` (a pool built with pair=True): the request's own second
        condition and its own two scales -- the result of `sample()` under `cfg_pair(model_wrapper(..., guidance_scale=s),
        c2, scale2, nested)`.  `guidance_scale=` needs `pair=` there; 1.0 is fine.  Default: the wrapper's.
        `negative_condition=n, guidance_scale=s, neg_scale=w` (a pool built with perp_neg=True): the request's own negative
        prompt and its own two scales, either without the other -- the result of `sample()` under
        `cfg_perp_neg(model_wrapper(..., guidance_scale=s), n, w)`; w = 0 is refused.  Default: the wrapper's."""
        s = self._s
        perp = self._perp_params(guidance_scale, neg_scale, negative_condition, pair, condition2)
        pair = self._pair_params(guidance_scale, pair, condition2)
        if self._pn:                     # (the third condition and the two scales travel as the pair pool's do)
            pair, condition2 = perp, negative_condition
        guide = self._guidance(None if self._three else guidance_scale, guidance_rescale)
        apg = self._apg_params(apg)
        zero_star = self._zstar_choice(zero_star)
        if blend is not None:
            if not self._inp:
                raise NotImplementedError("slab pool: blend= -- mask-blend stages take the table in a pool built with "
                                          "request_pool(slots=..., inpaint=True) only")
            if not isinstance(blend, MaskBlend):
                raise NotImplementedError("slab pool: blend= takes a dpm_solver_amd.MaskBlend (any other correcting_xt_fn runs "
                                          "Python between stages; sample with sample())")
            if sde:
                raise NotImplementedError("slab pool: blend= with sde=True -- the table has no blend behind the noise epilogue; "
                                          "sample it with sample_sde()")
            if blend.intermediates is None and blend.noise is None:
                raise NotImplementedError("slab pool: MaskBlend(x0=..., noise=None) draws torch.randn per call, which a pool "
                                          "cannot reproduce; pass noise= (the fixed-noise re-noising of the known image)")
        if not sde and (seed is not None or generator is not None):
            raise ValueError("slab pool: `seed` / `generator` belong to an SDE request (sde=True)")
        self._refuse(method, sde, return_intermediate)
        if sde:
            _sde.check_solver(s, order)
            seed = _sde.resolve_seed(seed, generator)
            if torch.is_tensor(x):
                _sde.check_state(s, x)
        t_0 = 1. / s.noise_schedule.total_N if t_end is None else t_end
        t_T = s.noise_schedule.T if t_start is None else t_start
        assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
        with torch.no_grad():
            plan = s._sample_plan(x, steps, t_0, t_T, order, skip_type, 'multistep', lower_order_final, denoise_to_zero,
                                  solver_type, sde=bool(sde))
        return self._enqueue(x, plan, condition, unconditional_condition, seed if sde else None, blend, guide, apg, zero_star,
                             condition2, pair)

    def submit_unipc(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', variant='bh2',
                     corrector=True, lower_order_final=True, denoise_to_zero=False, return_intermediate=False,
                     condition=None, unconditional_condition=None, guidance_scale=None):
        """Admit a UniPC request: `sample_unipc()`'s arguments, checks and errors in its order, then the pool's; the two
        condition arguments and `guidance_scale` as for `submit`.  `corrector=False` (variant 'bh2') admits sample()'s
        multistep plan."""
        s = self._s
        guide = self._guidance(guidance_scale, None)
        _unipc.check_solver(s, order, variant)
        t_0, t_T = _unipc._times(s, t_start, t_end)
        self._refuse(return_intermediate=return_intermediate)
        if not torch.is_tensor(x):
            DV._require_gpu(x)
        _unipc.check_state(s, x)
        if not corrector:
            if variant != 'bh2':
                raise NotImplementedError("sample_unipc: corrector=False with variant='bh1' (the predictor alone is built for "
                                          "'bh2', where it is DPM-Solver++ 2M)")
            return self.submit(x, steps=steps, t_start=t_start, t_end=t_end, order=order, skip_type=skip_type,
                               lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero, solver_type='dpmsolver',
                               condition=condition, unconditional_condition=unconditional_condition,
                               guidance_scale=guidance_scale)
        with torch.no_grad():
            plan = s._sample_plan(x, steps, t_0, t_T, order, skip_type, 'multistep', lower_order_final, denoise_to_zero,
                                  'dpmsolver', unipc=variant)
        return self._enqueue(x, plan, condition, unconditional_condition, guide=guide)

    def _conditions(self, b, cond, uncond, cond2=None):
        """the request's condition tensors, checked against the wrapper's guidance kind (None where the network takes none)"""
        w = self._s._wrapped
        if w is None or w.guidance_type != "classifier-free":
            if cond is not None or uncond is not None:
                raise ValueError("slab pool: `condition` / `unconditional_condition` belong to a classifier-free wrapper")
            return None, None, None
        cfg = w.effective_guidance == "classifier-free" or self._three
        cond = w.condition if cond is None else cond
        uncond = (w.unconditional_condition if uncond is None else uncond) if cfg else None
        cond2 = (w.pair[0] if cond2 is None else cond2) if self._three else None
        third = "negative_condition" if self._pn else "condition2"
        for name, c in (("condition", cond), ("unconditional_condition", uncond), (third, cond2)):
            if c is None and (name == "condition" or (cfg and name != third) or self._three):
                raise ValueError("slab pool: the request has no %s and the wrapper has none" % name)
            if c is not None and (not torch.is_tensor(c) or c.dim() < 1 or c.shape[0] not in (1, b)):
                raise ValueError("slab pool: %s must be a tensor of leading dimension %d or 1" % (name, b))
        if uncond is not None and (uncond.shape[1:] != cond.shape[1:] or uncond.dtype != cond.dtype):
            raise ValueError("slab pool: condition and unconditional_condition differ in shape or dtype")
        if cond2 is not None and (cond2.shape[1:] != cond.shape[1:] or cond2.dtype != cond.dtype):
            raise ValueError("slab pool: condition and %s differ in shape or dtype" % third)
        return cond, uncond, cond2

    def _blend_of(self, mb, x, plan, sd):
        """the request's `_Blend`: everything a tick must not compute per request, once, in the state dtype and contiguous"""
        shape, dev, es = tuple(x.shape), x.device, _esize(sd)
        b, per = int(shape[0]), self._per
        q = _Blend()
        m, period = mb._mask_for(shape, sd, dev)
        if period > per:                 # a full-size mask: sample k has its own `per` elements
            q.mstep, q.period = per * es, per
        else:
            if period % 8 != 0:          # a period the vector path cannot take: the full sample
                m, period = m.reshape(-1).repeat(per // period), per
            q.mstep, q.period = 0, period
        q.mask, q.keep = m, [m]
        n = len(plan.stages)
        q.rec = np.zeros(n, dtype=_BLEND)
        ops = {}

        def dense(t):                    # as MaskBlend.operands brings its tensors to the state
            t = t.to(device=dev, dtype=sd)
            return (t.expand(shape) if tuple(t.shape) != shape else t).contiguous()

        # where the blends are looked up: every stage that emits a state, at its (t_out, outer_step), then x_T at (stage 0's
        # t_eval, 0) -- run_plan at i == 0: blend.apply(state, t_eval, 0)
        emit = [i for i, ps in enumerate(plan.stages) if ps.emits_state]
        r = np.zeros(len(emit) + 1, dtype=_BLEND)
        r["flag"] = L.F_BLEND
        if mb.intermediates is not None:         # DiffEdit: the tensor of the step, as it is
            steps = [plan.stages[i].outer_step for i in emit] + [0]
            for step in steps:
                if step not in ops:
                    ops[step] = mb.intermediates[step].to(device=dev, dtype=sd).contiguous()
                    if tuple(ops[step].shape) != shape:
                        raise ValueError("slab pool: intermediates[%d] of shape %s for a state of %s"
                                         % (step, tuple(ops[step].shape), shape))
            r["alpha"], r["a"] = 1.0, [ops[step].data_ptr() for step in steps]
            q.first = (ops[0], None, 1.0, 0.0)
        else:                                    # the known image at the level of time_fn(t): MaskBlend._alpha_sigma, with
            ops["a"], ops["b"] = dense(mb.x0), dense(mb.noise)     # time_fn once per entry and ONE schedule evaluation each
            ts = [float(plan.stages[i].t_out) for i in emit] + [float(plan.stages[0].t_eval)]
            tt = np.array(ts if mb.time_fn is None else [float(mb.time_fn(t)) for t in ts], dtype=np.float32)
            r["alpha"] = mb.noise_schedule._eval_np(L.EVAL_ALPHA, tt)
            r["sigma"] = mb.noise_schedule._eval_np(L.EVAL_STD, tt)
            r["a"], r["b"] = ops["a"].data_ptr(), ops["b"].data_ptr()
            q.first = (ops["a"], ops["b"], float(r["alpha"][-1]), float(r["sigma"][-1]))
        q.rec[emit] = r[:-1]
        q.keep += list(ops.values())
        return q

    def _enqueue(self, x, plan, cond, uncond, seed=None, blend=None, guide=None, apg=None, zstar=None, cond2=None, pair=None):
        like, sd = self._check_state(x)
        if plan.slots > 3:
            raise NotImplementedError("slab pool: a plan with %d cached model values (the pool holds three)" % plan.slots)
        cond, uncond, cond2 = self._conditions(int(x.shape[0]), cond, uncond, cond2)
        if self._like is None:
            self._allocate(like, sd, cond)
        elif cond is not None and (tuple(cond.shape[1:]), cond.dtype) != (tuple(self._cslab.shape[1:]), self._cslab.dtype):
            raise ValueError("slab pool: a condition of shape %s, dtype %s does not match the pool's %s, %s"
                             % (tuple(cond.shape[1:]), cond.dtype, tuple(self._cslab.shape[1:]), self._cslab.dtype))
        q = _Waiting()
        q.h, q.x, q.plan, q.cond, q.uncond, q.mf, q.seed = self._next, x, plan, cond, uncond, DV._mf_of(x), seed
        q.blend = None if blend is None else self._blend_of(blend, x, plan, sd)
        q.guide, q.apg, q.zstar, q.cond2, q.pair = guide, apg, zstar, cond2, pair
        self._next += 1
        self._wait.append(q)
        return q.h

    # ------------------------------------------------------------------------------------------------------------------
    # storage
    # ------------------------------------------------------------------------------------------------------------------
    def _allocate(self, like, sd, cond):
        s, S = self._s, self.S
        shape, _, dev = like
        self._like, self._sd = like, sd
        w = s._wrapped
        self._cfg = w is not None and w.effective_guidance == "classifier-free"
        self._copies = 3 if self._three else 2 if self._cfg else 1  # copies of a state the network's input holds
        self._nS = nS = self._copies * S
        self._per = per = int(np.prod(shape, dtype=np.int64)) if shape else 1
        self._rowb = per * _esize(sd)
        self._x = [torch.zeros((nS,) + shape, dtype=sd, device=dev) for _ in range(2)]
        self._hist = [torch.zeros((S,) + shape, dtype=sd, device=dev) for _ in range(3)]
        self._hbase = np.array([t.data_ptr() for t in self._hist], dtype=np.uint64)
        if self._apg:
            self._avg = torch.zeros((S,) + shape, dtype=torch.float32, device=dev)
        self._cur = 0
        self._cslab = None
        if cond is not None:
            self._cslab = torch.zeros((nS,) + tuple(cond.shape[1:]), dtype=cond.dtype, device=dev)
        # staging: per ring slot a pinned buffer [table | next tick's times | this tick's times | stage array | buffers array]
        # and a device buffer for its first two parts (and one for the third: the copy an admitting tick adds)
        self._tabb = (L.table_bytes(S, self._tflags) + 15) // 16 * 16
        self._copyb = self._tabb + 4 * nS
        o_cur = (self._copyb + 15) // 16 * 16
        o_st = (o_cur + 4 * nS + 15) // 16 * 16
        o_bs = o_st + S * _STAGE.itemsize
        self._ring = []
        for _ in range(_RING):
            g = _Slot()
            g.pin, g.ev = DV._pinned_bytes(o_bs + S * _BUFS.itemsize), None
            g.dev, g.devt = DV._device_bytes(self._copyb, dev), DV._device_bytes(4 * nS, dev)
            a = g.pin.numpy()
            g.t_next, g.t_cur = a[self._tabb:self._copyb].view(np.float32), a[o_cur:o_cur + 4 * nS].view(np.float32)
            g.st, g.bufs, g.bufs_raw = a[o_st:o_bs].view(_STAGE), a[o_bs:].view(_BUFS), a[o_bs:]
            g.pin_cur = g.pin[o_cur:o_cur + 4 * nS]
            self._ring.append(g)
        self._t_attr = "t_input" if w is not None else "t_eval"

    def _plan_offset(self, plan):
        hit = self._plans.get(id(plan))
        if hit is None:
            n = len(plan.stages)
            arr = (L.Stage * n)(*[self._s._prep_stage(st.copy()) for st in plan.stages])
            hit = (len(self._recs), plan)
            self._recs = np.concatenate([self._recs, np.frombuffer(arr, dtype=_STAGE).copy()])
            self._plans[id(plan)] = hit
        return hit[0]

    def _admit(self):
        """waiting requests, first in first out, into free rows: their x_T (both halves under guidance) and conditions.
        Returns the inpainting requests among them as (rows, _Blend): their x_T is blended after the tick's network call."""
        taken = []
        while self._wait and int(self._wait[0].x.shape[0]) <= len(self._free):
            b = int(self._wait[0].x.shape[0])
            taken.append((self._wait.pop(0), self._free[:b]))
            self._free = self._free[b:]
        if taken:                        # whatever the rows' last requests left: gone, field by field of _ROW
            ra = np.array([r for _, rows in taken for r in rows], dtype=np.int64)
            for col, idle in self._cols:
                col[ra] = idle
            if self._apg:
                self._apg_reset(ra)
        blends = []
        for q, rows in taken:
            self._load_rows(q, rows)
            ra = np.asarray(rows, dtype=np.int64)
            self._off[ra], self._pos[ra], self._len[ra], self._req[ra] = self._plan_offset(q.plan), 0, len(q.plan.stages), q.h
            self._samp[ra] = np.arange(len(rows), dtype=np.int32)
            if q.seed is not None:
                self._sde_admit(q, ra)
            if q.guide is not None:
                self._guide_admit(q, ra)
            if self._apg:
                self._apg_admit(q, ra)
            if q.zstar is not None:
                self._zstar_admit(q, ra)
            if self._three:
                self._pair_admit(q, ra)
            if q.blend is not None:
                self._blend_admit(q, rows, ra)
                blends.append((rows, q.blend))
            self._rows[q.h] = (rows, q.mf)
        return blends

    def _load_rows(self, q, rows):
        """the request's x_T into its rows of the current state slab (both halves under guidance, all three thirds under
        guidance over two conditions), its conditions into the condition slab's: one copy per run of consecutive rows"""
        S, cur = self.S, self._x[self._cur]
        half = S if self._copies > 1 else 0   # the condition slab's conditional part (the unconditional one comes first)
        x = q.x.to(self._sd)
        k = 0
        for r0, cnt in _runs(rows):
            cur[r0:r0 + cnt].copy_(x[k:k + cnt])
            for part in range(1, self._copies):
                cur[part * S + r0:part * S + r0 + cnt].copy_(x[k:k + cnt])
            if q.cond2 is not None:
                c2 = q.cond2.to(self._cslab.device)
                self._cslab[2 * S + r0:2 * S + r0 + cnt].copy_(c2 if c2.shape[0] == 1 else c2[k:k + cnt])
            if q.cond is not None:
                c = q.cond.to(self._cslab.device)
                self._cslab[half + r0:half + r0 + cnt].copy_(c if c.shape[0] == 1 else c[k:k + cnt])
            if q.uncond is not None:
                u = q.uncond.to(self._cslab.device)
                self._cslab[r0:r0 + cnt].copy_(u if u.shape[0] == 1 else u[k:k + cnt])
            k += cnt

    def _network(self, x, t):
        """ONE call on the whole slab: the raw output(s) as (e0, e1, e2), e1 the unconditional part under guidance, e2 the
        part under the second condition of a pair=True pool (WrappedModel.raw_outputs' order)"""
        s = self._s
        w = s._wrapped
        if w is None:
            return s._model_fn(x, t), None, None
        if w.guidance_type != "classifier-free":
            return w.model(x, t, **w.model_kwargs), None, None
        out = w.model(x, t, self._cslab, **w.model_kwargs)
        if self._three:
            e1, e0, e2 = out.chunk(3)
            return e0, e1, e2
        if not self._cfg:
            return out, None, None
        e1, e0 = out.chunk(2)
        return e0, e1, None

    def _times_of(self, rows, idx):
        """the [S] (or [2S]) model-time vector of a tick whose active `rows` stand at the records `idx`; idle rows take the
        first active row's time (their output is ignored)"""
        t = np.empty(self._nS, dtype=np.float32)
        ta = self._recs[self._t_attr][idx]
        t[:] = ta[0] if len(ta) else 0.
        t[rows] = ta
        for part in range(1, self._copies):
            t[part * self.S + rows] = ta
        return t

    # ------------------------------------------------------------------------------------------------------------------
    # SDE requests.  Row fields: optp, seed (and samp, which every row has).  Kept per request: _ropts.
    # ------------------------------------------------------------------------------------------------------------------
    def _sde_admit(self, q, ra):
        """the request's own options (the solver's + its seed), kept while it is active; its rows point at them"""
        o = self._ropts[q.h] = _sde.request_opts(q.seed, self._s._opts_ptr())
        self._optp[ra], self._seed[ra] = C.addressof(o), np.uint64(q.seed)

    def _sde_tick(self, b, rows, rec):
        """the rows' own options; sample k's z starts at element k * per_sample; row 0's options are the call's: they carry
        its seed"""
        own = self._optp[rows]
        b["opts"] = np.where(own != 0, own, b["opts"])
        b["noise_sample0"] = np.where((rec["flags"] & L.F_NOISE) != 0, self._samp[rows], 0)
        seed0 = int(self._seed[rows[0]]) if own[0] else 0
        self._opts.noise_seed_lo, self._opts.noise_seed_hi = seed0 & 0xffffffff, seed0 >> 32

    def _sde_retire(self, h):
        self._ropts.pop(h, None)

    # ------------------------------------------------------------------------------------------------------------------
    # per-request guidance (any classifier-free pool).  Row fields: gon, gs, gphi.  Checked at submit: _guidance.
    # ------------------------------------------------------------------------------------------------------------------
    def _guide_admit(self, q, ra):
        self._gon[ra] = True
        self._gs[ra], self._gphi[ra] = q.guide

    def _guide_tick(self, st, rows, rec):
        """rows whose request brought its own guidance: what the planner and _bind_rescale write for a wrapper of that scale
        and phi (phi 0: no flag, a plain row), over the gathered records"""
        on = self._gon[rows] & (rec["guidance"] == L.GUIDE["classifier-free"])
        cs, cg, fl = DV._cfg_fields(self._gs[rows], self._gphi[rows], rec["sigma_e"], rec["flags"])
        st["cfg_scale"] = np.where(on, cs, rec["cfg_scale"])
        st["cg_scale"] = np.where(on, cg, rec["cg_scale"])
        st["flags"] = np.where(on, fl, rec["flags"])

    # ------------------------------------------------------------------------------------------------------------------
    # adaptive projected guidance (an apg=True pool).  Row fields: aon, aeta, ar, abeta.  Checked at submit: _apg_params.
    # Kept by the pool: _avg, the running averages, row by row.
    # ------------------------------------------------------------------------------------------------------------------
    def _apg_reset(self, ra):
        """a request starts from a zero average, whoever used its rows before: one zero_() per run of consecutive rows among
        the rows this tick admits"""
        for r0, cnt in _runs(sorted(ra.tolist())):
            self._avg[r0:r0 + cnt].zero_()

    def _apg_admit(self, q, ra):
        """the request's own parameters, or the wrapper's ((1, 0, 0): it has none)"""
        own = q.apg if q.apg is not None else self._s._remedy_setting("cfg_apg")
        self._aon[ra] = q.apg is not None
        self._aeta[ra], self._ar[ra], self._abeta[ra] = own if own is not None else (1.0, 0.0, 0.0)

    def _apg_tick(self, st, rows, rec):
        """rows whose request brought its own parameters or its own guidance scale: what _bind_apg writes for a wrapper of the
        row's parameters over the plain record of the row's scale ((1, 0, 0): no flag, a plain row), over the gathered records.
        Every other row keeps what _prep_stage bound."""
        on = (self._aon[rows] | self._gon[rows]) & (rec["guidance"] == L.GUIDE["classifier-free"])
        s = self._s                      # (the plain record: the planner's cg_scale of the row's scale, the solver's two fields)
        plain = (st["cfg_scale"] * rec["sigma_e"], np.float32(s.dynamic_thresholding_ratio), np.float32(s.thresholding_max_val))
        cg, ratio, mx, fl = DV._apg_fields(self._aeta[rows], self._ar[rows], self._abeta[rows], plain, st["flags"])
        st["cg_scale"] = np.where(on, cg, st["cg_scale"])
        st["thr_ratio"] = np.where(on, ratio, st["thr_ratio"])
        st["thr_max"] = np.where(on, mx, st["thr_max"])
        st["flags"] = np.where(on, fl, st["flags"])

    def _apg_buffers(self, st, b, rows):
        """the running average of a DPM_TABLE_APG call is thr_hint: the row's slice of the slab where its record has a
        momentum, 0 elsewhere"""
        mom = ((st["flags"] & np.uint32(L.F_CFG_APG)) != 0) & (st["thr_max"] != 0)
        b["thr_hint"] = np.where(mom, np.uint64(self._avg.data_ptr()) + rows.astype(np.uint64) * np.uint64(self._per * 4),
                                 np.uint64(0))

    # ------------------------------------------------------------------------------------------------------------------
    # CFG-Zero* (a zero_star=True pool).  Row fields: zon, zsel.  Checked at submit: _zstar_choice.  Nothing is kept by the
    # pool: the kind has no parameter and no state.
    # ------------------------------------------------------------------------------------------------------------------
    def _zstar_admit(self, q, ra):
        self._zon[ra], self._zsel[ra] = True, q.zstar

    def _zstar_tick(self, st, rows, rec):
        """rows whose request brought its own choice: what _bind_zstar writes for a wrapper with the setting (DPM_F_CFG_ZSTAR
        on a classifier-free record) or leaves for one without (no flag, a plain row), over the gathered records.  Every
        other row keeps what _prep_stage bound."""
        on = self._zon[rows] & (rec["guidance"] == L.GUIDE["classifier-free"])
        z = np.uint32(L.F_CFG_ZSTAR)
        st["flags"] = np.where(on, np.where(self._zsel[rows], st["flags"] | z, st["flags"] & ~z), st["flags"])

    # ------------------------------------------------------------------------------------------------------------------
    # guidance over two conditions (a pair=True pool) and Perp-Neg (a perp_neg=True pool: the same slabs, rows and records; s in
    # ps1, w in ps2, DPM_F_CFG2_PERP in the records' flags as _prep_stage bound it).  Row fields: ps1, ps2.  Checked at submit: _pair_params.  Nothing else is
    # kept by the pool: the kind has no state; its third output and third copy are pointers of the tick (_buffer_records).
    # ------------------------------------------------------------------------------------------------------------------
    def _pair_admit(self, q, ra):
        """the request's own two scales, or the wrapper's"""
        self._ps1[ra], self._ps2[ra] = q.pair if q.pair is not None else self._s._pair_setting()

    def _pair_tick(self, st, rows, rec):
        """every row's two scales over the gathered records, as the planner (cfg_scale = s1) and _prep_stage (cg_scale = s2)
        write them for a wrapper of the row's scales"""
        on = rec["guidance"] == L.GUIDE["classifier-free-2"]
        st["cfg_scale"] = np.where(on, self._ps1[rows], rec["cfg_scale"])
        st["cg_scale"] = np.where(on, self._ps2[rows], rec["cg_scale"])

    # ------------------------------------------------------------------------------------------------------------------
    # inpainting requests.  Row fields: bslot, bmask, bper (and samp).  Kept per request: _blends (built at submit: _blend_of)
    # and its records in _brec.
    # ------------------------------------------------------------------------------------------------------------------
    def _blend_admit(self, q, rows, ra):
        """the request's blend records at its first row; sample k of the request sits in rows[k]: its mask starts at element
        k * mstep"""
        bl = self._blends[q.h] = q.blend
        if self._brec.shape[1] < len(bl.rec):
            grown = np.zeros((self.S, len(bl.rec)), dtype=_BLEND)
            grown[:, :self._brec.shape[1]] = self._brec
            self._brec = grown
        self._brec[rows[0], :len(bl.rec)] = bl.rec
        self._bslot[ra], self._bper[ra] = rows[0], bl.period
        self._bmask[ra] = np.uint64(bl.mask.data_ptr()) + np.arange(len(rows), dtype=np.uint64) * np.uint64(bl.mstep)

    def _blend_first(self, blends, xin, stream):
        """x_T of the inpainting requests admitted on this tick, blended in the current state slab as run_plan blends it at
        i == 0 -- after the network has seen it.  One dpm_blend_launch per run of consecutive rows, through a temporary (the
        kernel's x and out are __restrict__: not in place); both halves under guidance."""
        S, per, rowb, code = self.S, self._per, self._rowb, DV._DT[self._sd]
        for rows, bl in blends:
            a, bb, alpha, sigma = bl.first
            k = 0
            for r0, cnt in _runs(rows):
                tmp = torch.empty_like(xin[r0:r0 + cnt])
                full = bl.mstep != 0
                L.check(DV._blend_launch_raw(xin[r0:r0 + cnt].data_ptr(), bl.mask.data_ptr() + k * bl.mstep,
                                             a.data_ptr() + k * rowb, None if bb is None else bb.data_ptr() + k * rowb,
                                             alpha, sigma, tmp.data_ptr(), cnt * per, cnt * per if full else bl.period, code,
                                             stream))
                xin[r0:r0 + cnt].copy_(tmp)
                if self._cfg:
                    xin[S + r0:S + r0 + cnt].copy_(tmp)
                k += cnt

    def _blend_tick(self, st, b, rows):
        """blend rows: DPM_F_BLEND, the scalars and the pointers of (request, position), sample k at base + k * stride"""
        slot = self._bslot[rows]
        width = self._brec.shape[1]
        br = (self._brec[np.clip(slot, 0, None), np.minimum(self._pos[rows], width - 1)] if width
              else np.zeros(len(rows), dtype=_BLEND))
        on = (slot >= 0) & (br["flag"] != 0)
        kb = self._samp[rows].astype(np.uint64) * np.uint64(self._rowb)
        st["flags"] |= np.where(on, br["flag"], 0).astype(np.uint32)
        st["blend_alpha"] = np.where(on, br["alpha"], np.float32(0))
        st["blend_sigma"] = np.where(on, br["sigma"], np.float32(0))
        b["mask"] = np.where(on, self._bmask[rows], np.uint64(0))
        b["blend_a"] = np.where(on, br["a"] + kb, np.uint64(0))
        b["blend_b"] = np.where(on & (br["b"] != 0), br["b"] + kb, np.uint64(0))
        b["mask_period"] = np.where(on, self._bper[rows], 0)

    def _blend_retire(self, h):
        self._blends.pop(h, None)

    # ------------------------------------------------------------------------------------------------------------------
    # one tick: step() and its phases, in the order they run
    # ------------------------------------------------------------------------------------------------------------------
    def step(self):
        """One stage of every active row: one network call, one table launch.  Returns {handle: result} of the requests that
        finished, fresh tensors in the layout of their x_T."""
        done = {}
        if self._like is None or not (self._rows or self._wait):
            return done
        stream, idx_dev, capturing, other = DV._launch_ctx(self._like[2])
        if capturing:
            raise RuntimeError("slab pool: ticks are not captured into graphs")
        with torch.no_grad():
            admitted = self._admit()
            rows = np.flatnonzero(self._req >= 0)
            R = len(rows)
            if R == 0:
                return done
            g = self._ring[self._tick % _RING]
            self._tick += 1
            DV._event_wait(g.ev)
            idx = self._off[rows] + self._pos[rows]
            rec = self._recs[idx]
            last = self._pos[rows] + 1 == self._len[rows]
            xin, xout = self._x[self._cur], self._x[1 - self._cur]
            e0, e1, e2, ed = self._bind(*self._network(xin if self._copies > 1 else xin[:self.S], self._tick_times(g, rows, idx)))
            if admitted:
                with DV._on_device(idx_dev, other):
                    self._blend_first(admitted, xin, stream)
            # the tick's records, vectorised: stage r = the record of row rows[r] at its position, pointers = base + row * stride
            st, b = g.st[:R], g.bufs[:R]
            st[:] = rec
            if self._cfg:
                self._guide_tick(st, rows, rec)
            if self._apg:
                self._apg_tick(st, rows, rec)
            if self._zst:
                self._zstar_tick(st, rows, rec)
            if self._three:
                self._pair_tick(st, rows, rec)
            self._buffer_records(g, b, rows, rec, last, xin, xout, e0, e1, ed, e2)
            if self._apg:
                self._apg_buffers(st, b, rows)
            self._call_opts(b)
            if self._sde:
                self._sde_tick(b, rows, rec)
            if self._inp:
                self._blend_tick(st, b, rows)
            b["opts"][0] = C.addressof(self._opts)
            # next tick's time vector rides with this tick's table
            t_next = self._times_of(rows[~last], idx[~last] + 1)
            g.t_next[:] = t_next
            with DV._on_device(idx_dev, other):
                rc = self._fill_copy_launch(g, b, R, stream)
            if rc:
                L.check(rc)
            del e0, e1, e2
            self._t_next, self._t_dev = t_next, g.dev[self._tabb:self._copyb].view(torch.float32)
            self._cur = 1 - self._cur
            self._pos[rows] += 1
            self._retire(rows[last], xout, done)
        return done

    def _tick_times(self, g, rows, idx):
        """the device's model-time vector of this tick: the one that rode with the previous tick's table, unless rows were
        admitted since -- then a copy of its own from ring slot `g`"""
        t_now = self._times_of(rows, idx)
        if self._t_dev is not None and np.array_equal(t_now, self._t_next):
            return self._t_dev
        g.t_cur[:] = t_now
        DV._copy_to_device(g.devt, g.pin_cur)
        self.copies += 1
        return g.devt.view(torch.float32)

    def _bind(self, e0, e1, e2=None):
        """the network's output as dense slabs of a dtype the kernels pair with the state's (launch_list._bind_outputs)"""
        sd = self._sd
        want = (self.S,) + self._like[0]
        if tuple(e0.shape) != want:
            raise NotImplementedError("slab pool: a network output of shape %s for an input of %s (channel slices of a wider "
                                      "output are not bound per row)" % (tuple(e0.shape), want))
        if e0.dtype is torch.float64 and self._s._state_dtype is None:
            raise NotImplementedError("slab pool: a double network output promotes the state to double")
        ed = e0.dtype
        if ed is not sd and (sd is not torch.float32 or ed not in DV._DT):
            ed = sd
        e0 = DV._conv(e0, ed)
        e1 = DV._conv(e1, ed)
        e2 = DV._conv(e2, ed)
        return e0, e1, e2, ed

    def _buffer_records(self, g, b, rows, rec, last, xin, xout, e0, e1, ed, e2=None):
        """the rows' dpm_buffers, zeroed and filled: every pointer is base + row * stride, a history slot the record names"""
        g.bufs_raw[:len(rows) * _BUFS.itemsize] = 0
        rb = rows.astype(np.uint64) * np.uint64(self._rowb)
        eb = rows.astype(np.uint64) * np.uint64(self._per * e0.element_size())
        b["x"] = np.uint64(xin.data_ptr()) + rb
        b["x_out"] = np.uint64(xout.data_ptr()) + rb
        if self._cfg:
            b["x_out2"] = np.where(last, np.uint64(0), np.uint64(xout.data_ptr() + self.S * self._rowb) + rb)
            b["e1"] = np.uint64(e1.data_ptr()) + eb
        if self._three:                  # the third output, and the other two thirds of the network's next input
            b["e1"] = np.uint64(e1.data_ptr()) + eb
            b["g"] = np.uint64(e2.data_ptr()) + eb
            b["x_out2"] = np.where(last, np.uint64(0), np.uint64(xout.data_ptr() + self.S * self._rowb) + rb)
            b["thr_hint"] = np.where(last, np.uint64(0), np.uint64(xout.data_ptr() + 2 * self.S * self._rowb) + rb)
        b["e0"] = np.uint64(e0.data_ptr()) + eb
        for name, slot, used in (("h1", rec["h1_slot"], rec["h1_slot"] >= 0), ("h2", rec["h2_slot"], rec["h2_slot"] >= 0),
                                 ("m_out", rec["m_slot"], (rec["flags"] & L.F_STORE_M) != 0)):
            b[name] = np.where(used, self._hbase[np.clip(slot, 0, 2)] + rb, np.uint64(0))
        b["n"], b["batch"] = self._per, 1
        b["state_dtype"], b["eps_dtype"] = DV._DT[self._sd], DV._DT[ed]

    def _call_opts(self, b):
        """the call's options: a copy of the solver's with per-request stages and no seed (an SDE row 0 brings its own:
        _sde_tick); every row points at the solver's, row 0 -- once the kinds have written theirs -- at the copy"""
        o = self._s._opts_ptr()
        if o is not None:
            C.memmove(C.byref(self._opts), o, C.sizeof(L.LaunchOpts))
            b["opts"] = C.addressof(o.contents)
        self._opts.per_request_stages, self._opts.fuse_shapes = 1, 0
        self._opts.noise_seed_lo = self._opts.noise_seed_hi = 0

    def _fill_copy_launch(self, g, b, R, stream):
        """DPM_TABLE_FILL into ring slot `g`'s pinned buffer, its ONE copy (the table and the next tick's times), DPM_TABLE_LAUNCH
        on the device's; returns the library's error code, table_mode 0 again either way"""
        flag, pin, dev = self._tflags, g.pin, g.dev
        sts = C.cast(g.st.ctypes.data, C.POINTER(L.Stage))
        bufs = C.cast(g.bufs.ctypes.data, C.POINTER(L.Buffers))
        self._opts.table_mode = L.TABLE_FILL | flag
        b["workspace"][0] = pin.data_ptr()
        rc = DV._stage_launch_multi_raw(sts, bufs, R, stream)
        if rc == 0:
            g.ev = DV._copy_to_device(dev, pin[:self._copyb])
            self.copies += 1
            self._opts.table_mode = L.TABLE_LAUNCH | flag
            b["workspace"][0] = dev.data_ptr()
            rc = DV._stage_launch_multi_raw(sts, bufs, R, stream)
        self._opts.table_mode = 0
        return rc

    def _retire(self, rows, xout, done):
        """the requests of the finished `rows` into `done`: their rows, cloned from the output slab, are free again"""
        for h in np.unique(self._req[rows]).tolist():
            rws, mf = self._rows.pop(h)
            self._sde_retire(h)
            self._blend_retire(h)
            parts = [xout[r0:r0 + cnt] for r0, cnt in _runs(rws)]
            out = parts[0].clone() if len(parts) == 1 else torch.cat(parts)
            done[h] = out if mf is None else DV._conv(out, out.dtype, mf)
            self._req[np.asarray(rws, dtype=np.int64)] = -1
            self._free = sorted(self._free + rws)
