"""DPM_Solver -- host mirror of the reference class (dpm_solver_pytorch.py:337-1245).

Same constructor, same `.sample()` / `.inverse()` / `.add_noise()` and the same public per-update
methods.  What differs is where the work happens:

  * every scalar of a sampling run is computed once by the C planner into a list of stages
    (`dpm_plan_create`); this class only walks that list;
  * per stage it calls the opaque network (PyTorch-ROCm, current stream) and then launches ONE fused
    HIP kernel through the C ABI (`dpm_stage_launch`) on the same stream;
  * there is no CPU path: tensors must live on an AMD GPU, and a missing library fails at import.

The class and its reference-named methods live here; what they run on is split by concern (round 6, no bit changed):

  _device.py      the device entry points (one dpm_stage_launch, the raw C entry points, add_noise, the error norm) and the
                  tensor-layout helpers -- the one namespace the CPU test double and the timing tools hook into
  plan_cache.py   `_Plan` (a frozen dpm_plan + its per-device time tensors) and the plan cache
  launch_list.py  `_FastRun` (prebuilt launch records of a sample() call), `_bind_outputs`
  loops.py        the three sampling loops: fast path, several requests per fused launch, the general loop with callbacks
  updates.py      the machinery under the public per-update methods
  adaptive.py     the adaptive solver: device-side controller, host loop, the predicate that chooses
  capture.py      hipGraph capture (`GraphedSample`) and auto_capture
  pool.py         `RequestPool`: continuous batching, one fused launch per tick for requests at any stage
  remedies.py     the classifier-free remedies (cfg_rescale, cfg_apg, cfg_zero_star) as one table: a kind's setting, binder,
                  refusals and pool switch are a row; `_remedies`, `_remedy_key` and `_check_remedies` read it

`ref :NNN` = line in the reference's dpm_solver_pytorch.py.
"""
import ctypes as C
import inspect

import sys
import types

import numpy as np
import torch

from . import _device as DV
from . import _lib as L
from . import adaptive as _adaptive
from . import capture as _capture
from . import loops as _loops
from . import plan_cache as _plan_cache
from . import pool as _pool
from . import remedies as _rem
from . import slab as _slab
from . import sde as _sde
from . import unipc as _unipc
from . import updates as _updates
from .capture import GraphedSample
from .correctors import MaskBlend  # noqa: F401  (part of this module's namespace since round 2)
from .launch_list import _FastRun, _bind_outputs  # noqa: F401
from .plan_cache import _Cloning, _Plan  # noqa: F401
from .wrapper import WrappedModel


class DPM_Solver:
    # Engine options (extensions; class-level defaults, settable per instance).
    # adaptive solver: controller on the device (no host synchronisation per iteration); False = the reference's host
    # loop (one .item() per iteration, ref :1002).  With the device controller the host enqueues `adaptive_lookahead`
    # iterations ahead of the device's decisions (clamped to 0..24): the lookahead + 1 iterations enqueued after t_end was
    # reached still call the network (their solver kernels are no-ops) -- the reported NFE and the result do not change,
    # the number of network calls is (lookahead + 1) * order larger than the reference's.
    adaptive_on_device = True
    adaptive_lookahead = 1
    # per-call launch options of the C ABI (dpm_launch_opts), handed to every launch of this solver:
    #   cluster_in_graph  dynamic thresholding keeps its workgroup clusters under hipGraph capture also for samples that fit
    #                     one workgroup (default: one workgroup per sample there -- a replayed graph runs outside the
    #                     library's per-device chain of clustered launches)
    #   thr_spin_limit    polls before a wait between the workgroups of a thresholding cluster gives up and the workgroup
    #                     finishes its sample alone (0 = the library's default, 4096: milliseconds)
    cluster_in_graph = False
    thr_spin_limit = 0
    # auto_capture = N > 0 (opt-in): after N sample() calls with the same arguments, shape, dtype and stream, the call is
    # hipGraph-captured (DPM_Solver.capture) and later calls replay the graph -- one launch per trajectory instead of one per
    # kernel, which is what a launch-bound loop needs ([8,4,64,64]: 98 -> 52 us per trajectory with a frozen network).  Not
    # the default: a replay does not re-run the PYTHON side of the network (counters, hooks, host-side control flow,
    # conditioning tensors swapped for new objects), which the reference's eager loop does at every call -- the caller has
    # to know its network is a pure function of (x, t) on fixed tensors, as for torch.cuda.graph.  Calls with Python callbacks
    # (correcting_xt_fn, a callable correcting_x0_fn), return_intermediate or a host-side adaptive loop are never captured.
    auto_capture = 0
    _noise_seed = None                       # sample_sde: the seed of the call in progress (dpm_launch_opts.noise_seed_*)
    _group_seeds = None                      # sample_sde_requests: the seeds of the group in progress, one per request
    _sde_opts = None

    def __init__(self, model_fn, noise_schedule, algorithm_type="dpmsolver++", correcting_x0_fn=None,
                 correcting_xt_fn=None, thresholding_max_val=1., dynamic_thresholding_ratio=0.995,
                 state_dtype=None):
        """Construct a DPM-Solver (signature of ref :338-347; `state_dtype` is an extension).

        state_dtype: dtype the solver keeps x and the cached model values in.  None follows the reference:
        with a 'discrete' schedule a half-precision x_T is promoted to fp32 by the first update (the
        reference's coefficients are (1,)-shaped fp32 tensors), with 'linear' it keeps x's dtype.
        """
        self.model = lambda x, t: model_fn(x, t.expand((x.shape[0])))
        self._model_fn = model_fn
        self._wrapped = model_fn if isinstance(model_fn, WrappedModel) else None
        self.noise_schedule = noise_schedule
        assert algorithm_type in ["dpmsolver", "dpmsolver++"]
        self.algorithm_type = algorithm_type
        self._thresholding = correcting_x0_fn == "dynamic_thresholding"
        if self._thresholding:
            self.correcting_x0_fn = self.dynamic_thresholding_fn
            self._user_x0 = None
        else:
            self.correcting_x0_fn = correcting_x0_fn
            self._user_x0 = correcting_x0_fn
        self._user_x0_nargs = None
        if self._user_x0 is not None:
            try:  # the older vendored revision calls correcting_x0_fn(x0) with one argument
                self._user_x0_nargs = len([p for p in inspect.signature(self._user_x0).parameters.values()
                                           if p.default is p.empty and p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)])
            except (TypeError, ValueError):
                self._user_x0_nargs = 2
        self.correcting_xt_fn = correcting_xt_fn
        self.dynamic_thresholding_ratio = dynamic_thresholding_ratio
        self.thresholding_max_val = thresholding_max_val
        self._state_dtype = state_dtype
        # The (batch,) time vectors handed to the network are built once per (plan, batch) and shared by every call
        # (the reference makes a fresh tensor per call, ref :404).  A network that writes into its time argument gets a
        # clone per call: fresh_time_tensors = True, switched on automatically when such a write is detected
        # (_Plan.time_views).
        self.fresh_time_tensors = False
        self._plans = {}
        self._auto = {}                      # auto_capture: (arguments, shape, ...) -> [calls seen, GraphedSample]
        self._fast = {}
        self._fast_groups = {}
        self._group = None                   # sample_requests: the requests advanced together by this call
        self._adaptive_handles = {}
        # adaptive solver: optional hook applied to the 0-dim batch-maximum error before the controller reads it
        self.error_reduce = None
        self.adaptive_max_iterations = None  # bound of the loop (required knowledge under hipGraph capture: default 64)

    # ------------------------------------------------------------------------------------------
    # helpers
    # ------------------------------------------------------------------------------------------
    @property
    def _h(self):
        return self.noise_schedule._h

    @property
    def _algo(self):
        return L.ALGO[self.algorithm_type]

    def _opts_ptr(self):
        """ctypes pointer to this solver's dpm_launch_opts, or None when everything is at its default"""
        key = (bool(self.cluster_in_graph), int(self.thr_spin_limit))
        if self._noise_seed is not None:
            seed = int(self._noise_seed)
            hit = self._sde_opts
            if hit is None or hit[0] != (key, seed):
                o = L.LaunchOpts()
                o.cluster_in_graph, o.thr_spin_limit = int(key[0]), key[1]
                o.noise_seed_lo, o.noise_seed_hi = seed & 0xffffffff, seed >> 32
                hit = self._sde_opts = ((key, seed), o, C.pointer(o))
            return hit[2]
        if key == (False, 0):
            return None
        hit = getattr(self, "_opts_cache", None)
        if hit is None or hit[0] != key:
            o = L.LaunchOpts()
            o.cluster_in_graph, o.thr_spin_limit = int(key[0]), key[1]
            hit = self._opts_cache = (key, o, C.pointer(o))
        return hit[2]

    def _model_codes(self):
        if self._wrapped is not None:
            w = self._wrapped
            return L.MODEL[w.model_type], L.GUIDE[w.effective_guidance], float(w.guidance_scale)   # (cfg_pair: s1 is the scale)
        return L.MODEL["noise"], L.GUIDE["uncond"], 1.0

    # the classifier-free remedies (cfg_rescale, cfg_apg, cfg_zero_star): one table, one face (dpm_solver_amd/remedies.py)
    _remedies = _rem.active
    _remedy_setting = _rem.setting
    _remedy_key = _rem.key
    _check_remedies = _rem.check

    # guidance over two conditions (cfg_pair; DPM_GUIDE_CFG2): its setting, its cache key, what it is not built with
    _PAIR = "guidance over two conditions (cfg_pair)"

    def _pair_setting(self):
        """(s1, s2) of the wrapper's cfg_pair, None = off"""
        p = self._wrapped.pair if self._wrapped is not None else None
        return None if p is None else (float(p[1]), float(p[2]))

    def _pair_key(self):
        """what the caches of plans, launch records and graphs key on besides _remedy_key(): changes with the pair setting.
        condition2 enters by IDENTITY, like the wrapper's own conditions in the graph cache's key (capture.auto_captured) and in
        its concatenated `_c_in`.  The wrapper holds the tensor, so no other tensor takes its id while the wrapper lives; what the
        key cannot see is an edit IN PLACE, or a `guidance_pair` assigned by hand.  Hence the rule (cfg_pair's docstring,
        INTEGRATION.md): a condition tensor is immutable for the life of its wrapper -- the concatenated conditions are built
        once and a captured graph keeps replaying them.  Another condition takes another cfg_pair(...) and another DPM_Solver."""
        p = self._wrapped.pair if self._wrapped is not None else None
        if p is None:
            return None
        key = (id(p[0]), float(p[1]), float(p[2]))
        return key + ("perp_neg",) if self._perp() else key     # (without cfg_perp_neg every key is what it was)

    def _perp(self):
        """does the wrapper ask for Perp-Neg (cfg_perp_neg; DPM_F_CFG2_PERP)?  _pair_setting() is then (s, w): the guidance and
        the negative scale, and every rule of _check_pair applies as it stands"""
        return self._wrapped is not None and self._wrapped.perp

    def _check_pair(self, what=None, blend=False):
        """The combinations guidance over two conditions is not built with.  `what` names a sampler or a mode without the
        three-branch kernel; else the solver-wide rules, then the run's corrector (`blend`)."""
        if self._pair_setting() is None:
            return
        if what is not None:
            raise NotImplementedError("%s: %s" % (self._PAIR, what))
        if self._thresholding:
            raise NotImplementedError("%s: correcting_x0_fn='dynamic_thresholding' -- the thresholding kernels blend two network "
                                      "outputs, not three (a follow-up)" % self._PAIR)
        if self._user_x0 is not None:
            raise NotImplementedError("%s: a callable correcting_x0_fn -- the split stage's prologue kernel blends two network "
                                      "outputs, not three (a follow-up)" % self._PAIR)
        if blend:
            raise NotImplementedError("%s: a MaskBlend corrector -- stage_pair_kernel has no mask-blend epilogue (a follow-up)"
                                      % self._PAIR)

    def _apg_average(self, shape, device):
        """a zeroed running average for one run under adaptive projected guidance with a momentum (fp32, the state's shape);
        None where the run carries none"""
        apg = self._remedy_setting("cfg_apg")
        if apg is None or apg[2] == 0.0:
            return None
        return torch.zeros(tuple(shape), dtype=torch.float32, device=device)

    def _sdtype(self, x):
        if self._state_dtype is not None:
            return self._state_dtype
        if x.dtype not in DV._DT:
            raise NotImplementedError("dpm_solver_amd: state dtype %s is not supported (fp64 / fp32 / fp16 / bf16)" % x.dtype)
        # torch's type promotion between x and the reference's (1,)-shaped coefficient tensors (ref :573-576), which have the
        # dtype of the schedule's tables for 'discrete' and of the time tensor (fp32) otherwise
        if x.dtype is torch.float64:
            return torch.float64
        if self.noise_schedule.schedule == 'discrete':
            return torch.float64 if getattr(self.noise_schedule, "dtype", torch.float32) == torch.float64 else torch.float32
        return x.dtype

    def _precision(self, sd):
        """1: the scalars of the run are doubles -- a double state on a 'discrete' schedule declared dtype=float64 (every
        coefficient of the reference is then a double tensor); 0: fp32 scalars (meeting a double state they are converted
        exactly, like the reference's fp32 coefficient tensors are by type promotion)"""
        ns = self.noise_schedule
        return int(sd is torch.float64 and ns.schedule == 'discrete' and getattr(ns, "dtype", torch.float32) == torch.float64)

    @staticmethod
    def _tf(t):
        """time argument (tensor of one element, or float) -> fp32 host value"""
        if torch.is_tensor(t):
            return float(t.detach().reshape(-1)[0].float().item())
        return float(DV._F32(t))

    def _tt(self, value, device, shape1=False, dtype=torch.float32):
        t = torch.full((1,) if shape1 else (), float(value), dtype=dtype, device=device)
        return t

    @staticmethod
    def _td(t):
        """time argument -> host double (exact for fp32 / fp64 tensors and Python floats)"""
        if torch.is_tensor(t):
            return float(t.detach().reshape(-1)[0].double().item())
        return float(t)

    def _double_call(self, x, *times):
        """(scalars are doubles, the time tensors are doubles) for a public per-update call: torch's type promotion makes
        every scalar of the reference a double when a time tensor is one or the schedule's tables are (ref :127-134)"""
        tf64 = any(torch.is_tensor(t) and t.dtype is torch.float64 for t in times)
        ns = self.noise_schedule
        return bool(tf64 or (ns.schedule == 'discrete' and getattr(ns, "dtype", torch.float32) == torch.float64)), tf64

    def _out_double(self, x, times=(), models=(), evaluates=False):
        """Is the RESULT of a public per-update call a double tensor?  (Whether its SCALARS are doubles is _double_call's
        question: a double time makes them so.)  torch's type promotion: x or a model value handed in is double; a coefficient
        is a DIMENSIONED double tensor -- every scalar of a 'discrete' schedule is (1,)-shaped (ref :130), on a continuous one
        a scalar has its time argument's shape, so a 0-dim double time does not promote an fp32 tensor; or a model evaluation
        inside the call converts with alpha_t / sigma_t of the time expanded to the batch (x_start / v / score, classifier)."""
        if self._sdtype(x) is torch.float64 or any(m is not None and m.dtype is torch.float64 for m in models):
            return True
        ns = self.noise_schedule
        disc = ns.schedule == 'discrete'
        if disc and getattr(ns, "dtype", torch.float32) == torch.float64:
            return True
        t64 = [t for t in times if torch.is_tensor(t) and t.dtype is torch.float64]
        if any(disc or t.dim() >= 1 for t in t64):
            return True
        if t64 and evaluates:
            mt, gd, _ = self._model_codes()
            return mt != L.MODEL["noise"] or gd == L.GUIDE["classifier"]
        return False

    def _call_sdtype(self, x, times=(), models=(), evaluates=False):
        """State dtype of ONE public per-update call (the fp32 / half side; doubles are _double_call's).  _sdtype(x), widened
        by what torch's type promotion does to the reference's expression: model values handed in by the caller take part
        as they are; and a half state on a CONTINUOUS schedule -- kept by 0-dim coefficients -- becomes fp32 as soon as a
        coefficient is a dimensioned tensor: a time argument of shape (1,) (ref :553-590: every scalar inherits its shape), or
        a model evaluation inside the call whose conversions multiply by alpha_t / sigma_t expanded to the batch (x_start / v /
        score networks, the classifier term: ref :290-298, :320)."""
        sd = self._sdtype(x)
        if self._state_dtype is not None:
            return sd
        for m in models:
            if m is not None and m.dtype in DV._DT and m.dtype is not torch.float64:
                sd = torch.promote_types(sd, m.dtype)
        if sd in (torch.float16, torch.bfloat16):
            wide = any(torch.is_tensor(t) and t.dim() >= 1 for t in times)
            if evaluates and not wide:
                mt, gd, _ = self._model_codes()
                wide = mt != L.MODEL["noise"] or gd == L.GUIDE["classifier"]
            if wide:
                sd = torch.float32
        return sd

    def _time_views(self, plan, device, batch, cfg):
        """plan.time_views; a network that was caught writing into the shared time vectors gets clones from now on.  Guidance
        over two conditions calls the network on three copies: its `t_input_2b` is the tripled time, built once like the doubled one"""
        V = plan.time_views(device, batch, 3 if self._pair_setting() is not None else cfg)
        if plan.times_written and not self.fresh_time_tensors:
            self.fresh_time_tensors = True
        return V

    def _call_x0(self, x0, t):
        if self._user_x0_nargs == 1:
            return self._user_x0(x0)
        return self._user_x0(x0, t)

    def _network(self, x_eval, t_eval_t, t_input_t, x_in2=None, pre=None):
        """the opaque call: raw output(s) of the network at (x_eval, t).  x_in2: [2B,...] buffer both halves of
        which already hold x_eval (written by the previous stage kernel) -- the CFG network input.  pre: the
        time tensors already expanded to the batch (t_eval_b, t_input_b, t_input_2b)."""
        B = x_eval.shape[0]
        if pre is not None:
            te, ti, t2 = pre
        else:
            te, ti = t_eval_t.expand(B), t_input_t.expand(B)
            eff = self._wrapped.effective_guidance if self._wrapped is not None else None
            t2 = t_input_t.expand(2 * B) if eff == "classifier-free" else t_input_t.expand(3 * B) if eff == "classifier-free-2" else None
        if self._wrapped is not None:
            return self._wrapped.raw_outputs(x_eval, te, ti, t2, x_in2=x_in2)
        return self._model_fn(x_eval, te), None, None

    def _promoted(self, sd, e0, plan=None):
        """State dtype after the first network evaluation.  Without an explicit `state_dtype` the reference's type
        promotion applies: a half-precision state combined with a network output of another floating dtype (fp32
        eps next to an fp16 x on a 'linear' schedule, or fp16 next to bf16) continues in fp32 from the first update on
        (ref :573-576 are plain tensor expressions).  An explicit `state_dtype` keeps the state there and the output
        is converted to it.

        A half state on a continuous schedule also leaves half precision when a singlestep update of order >= 2 runs: its
        intermediate time comes out of inverse_lambda, which for 'linear' builds a (1,)-shaped tensor (ref :161: `torch.zeros((1,))`)
        -- a dimensioned fp32 coefficient, and the state is fp32 from that update on (measured against the reference:
        tests/test_differential_reference.py).  The first such update is the trajectory's first or second, so the run continues
        in fp32 from its first update; the one deviation is that the reference rounds the FIRST model value to half once."""
        if self._state_dtype is None and e0.dtype is torch.float64:
            return torch.float64                    # a double network output promotes every state
        if self._state_dtype is None and sd not in (torch.float32, torch.float64) and e0.dtype is not sd and e0.dtype in DV._DT:
            return torch.float32
        if self._state_dtype is None and sd not in (torch.float32, torch.float64) and self.noise_schedule.schedule != 'discrete':
            if plan is not None and plan.has_inner_nodes:
                return torch.float32
            # ... and when the wrapped model's OWN conversions involve the schedule: x_start / v / score networks and the
            # classifier term multiply by alpha_t / sigma_t expanded to the batch (ref :290-298, :320: dimensioned fp32
            # tensors), so the noise the solver receives -- and every state after the first update -- is fp32
            mt, gd, _ = self._model_codes()
            if mt != L.MODEL["noise"] or gd == L.GUIDE["classifier"]:
                return torch.float32
        return sd

    def _cfg_pre(self, outs, sd):
        """Double state, classifier-free guidance, a noise-prediction network that answers in a narrower dtype: the reference
        blends `uncond + scale * (cond - uncond)` in the NETWORK's dtype (ref :326-330, a Python-float scale) before any double
        scalar touches the result.  The double kernel would blend in double, so the blend is taken here, in the reference's
        own expression, and handed on as both halves (e1 + s * (e0 - e1) with e0 == e1 is exact)."""
        e0, e1, g = outs
        pair = self._pair_setting()
        if sd is torch.float64 and pair is not None:
            # guidance over two conditions has no double kernel: the three raw outputs are blended here, in double, and handed
            # on as ONE unguided output (the conversions are affine in the output and the three weights sum to one, so blending
            # before them is the same function; the stage record is unguided then: _unguided64)
            e0, e1, g = e0.double(), e1.double(), g.double()
            if self._perp():
                # Perp-Neg likewise: projection and blend in double on the raw outputs (include/dpm_hip.h, DPM_F_CFG2_PERP)
                axes = list(range(1, e0.dim()))
                d0, d2 = e0 - e1, g - e1
                s_dd = (d0 * d0).sum(dim=axes, keepdim=True)
                a = torch.where(s_dd > 0, (d2 * d0).sum(dim=axes, keepdim=True) / s_dd, torch.zeros_like(s_dd))
                return e1 + pair[0] * (d0 - pair[1] * (d2 - a * d0)), None, None
            return (e1 + pair[0] * (e0 - e1)) + pair[1] * (g - e1), None, None
        if (sd is torch.float64 and e1 is not None and e0.dtype is not torch.float64 and self._wrapped is not None
                and self._wrapped.model_type == "noise"):
            e = e1 + self._wrapped.guidance_scale * (e0 - e1)
            return e, e, g
        return outs

    def _stage64(self, st, s64=None):
        """the dpm_stage_f64 of a launch on a double state: the double-precision plan's record, or -- fp32 scalars (an fp32
        schedule) -- the stage's floats converted exactly, as torch's type promotion converts the reference's fp32
        coefficient tensors; either way with the thresholding parameters as the doubles torch.quantile / torch.maximum make
        of the Python floats (ref :422-423)"""
        out = L.StageF64()
        if s64 is not None:
            C.memmove(C.byref(out), C.byref(s64), C.sizeof(L.StageF64))
        else:
            for f in ("t_eval", "t_input", "t_out", "alpha_e", "sigma_e", "cfg_scale", "cg_scale", "cx", "c0", "c1", "c2",
                      "blend_alpha", "blend_sigma"):
                setattr(out, f, float(getattr(st, f)))
            for j in range(5):
                out.k[j] = float(st.k[j])
        out.thr_ratio = float(self.dynamic_thresholding_ratio)
        out.thr_max = float(self.thresholding_max_val)
        return out

    def _unguided64(self, st, sd):
        """a double state under guidance over two conditions: _cfg_pre hands the stage ONE blended output -- its record is unguided"""
        if sd is torch.float64 and st.guidance == L.GUIDE["classifier-free-2"]:
            st.guidance = L.GUIDE["uncond"]
            st.flags &= ~L.F_CFG2_PERP                          # (the flag is valid under the guidance only)
        return st

    def _prep_stage(self, st):
        """stage flags and fields that depend on this solver's correctors and on its wrapper's remedy: per active kind its
        check, its refusal of a thresholded stage, its bind"""
        if st.flags & L.F_TO_X0:
            if self._thresholding:
                st.flags |= L.F_THRESH
                st.thr_ratio = float(self.dynamic_thresholding_ratio)
                st.thr_max = float(self.thresholding_max_val)
        for r, v in self._remedies():
            self._check_remedies(only=r.name)
            if st.flags & L.F_THRESH:
                raise _rem.thresholded(r)
            r.bind(st, v)
        if st.guidance == L.GUIDE["classifier-free-2"]:
            self._check_pair()
            st.cg_scale = self._pair_setting()[1]               # s2 (the planner wrote 0; cfg_scale is s1 already)
            if self._perp():
                st.flags |= L.F_CFG2_PERP                           # (cg_scale: the negative scale w)
        return st

    def _run_stage(self, st, x, xe, outs, h1, h2, sd, t_eval_t, want_m=None, ext=None, coef64=None):
        """outs = (e0, e1, g) fresh network outputs.  Handles a *callable* correcting_x0_fn by splitting the
        stage: prologue kernel -> user function (opaque torch) -> combination kernel."""
        self._check_remedies(sd=sd)         # (sd: possibly promoted by the first evaluation; st was bound by _prep_stage)
        e0, e1, g = outs if sd is not torch.float64 else self._cfg_pre(outs, sd)
        self._unguided64(st, sd)
        if self._user_x0 is not None and (st.flags & L.F_TO_X0):
            s1 = st.copy()
            s1.form = L.FORM_DENOISE
            s1.flags = L.F_TO_X0 | (st.flags & _rem.F_CFG_REMEDIES)
            avg = ext.get("apg_avg") if ext is not None else None
            x0, _ = DV._launch_stage(s1, None, xe if xe is not None else x, e0, e1, g, None, None, sd, want_m=False,
                                  ext={"apg_avg": avg} if avg is not None else None, opts=self._opts_ptr(), coef64=coef64)
            x0 = self._call_x0(x0, t_eval_t)                                             # ref :440-441
            return self._run_given(st, x, x0, h1, h2, sd, want_m, ext=ext, coef64=coef64)
        return DV._launch_stage(st, x, xe, e0, e1, g, h1, h2, sd, want_m=want_m, ext=ext, opts=self._opts_ptr(), coef64=coef64)

    def _run_given(self, st, x, m, h1, h2, sd, want_m=None, ext=None, coef64=None):
        """the update of `st` with the model value already known (no prologue)"""
        s2 = st.copy()
        s2.flags = st.flags & L.F_BASE_HIST
        s2.model_type = L.MODEL["noise"]
        s2.guidance = L.GUIDE["uncond"]
        store = bool(st.flags & L.F_STORE_M) if want_m is None else want_m
        x_out, _ = DV._launch_stage(s2, x if x is not None else m, None, m, None, None, h1, h2, sd, want_m=False, ext=ext,
                                 opts=self._opts_ptr(), coef64=coef64)
        return x_out, (m if store else None)

    # ------------------------------------------------------------------------------------------
    # model evaluations (ref :416-451, :541-545)
    # ------------------------------------------------------------------------------------------
    def dynamic_thresholding_fn(self, x0, t=None):
        """The dynamic thresholding method (ref :416-425) as one kernel launch."""
        DV._require_gpu(x0)
        st = L.Stage()
        st.h1_slot = st.h2_slot = st.m_slot = -1
        st.form = L.FORM_DENOISE
        st.flags = L.F_THRESH
        st.thr_ratio = float(self.dynamic_thresholding_ratio)
        st.thr_max = float(self.thresholding_max_val)
        st.alpha_e, st.sigma_e, st.cfg_scale = 1.0, 0.0, 1.0
        sd = x0.dtype if x0.dtype in DV._DT else torch.float32
        out, _ = DV._launch_stage(st, None, x0, x0, None, None, None, None, sd, want_m=False, opts=self._opts_ptr(),
                               coef64=self._stage64(st) if sd is torch.float64 else None)
        return out


    _eval_model = _updates.eval_model

    def noise_prediction_fn(self, x, t):
        """Return the noise prediction model (ref :427-431)."""
        return self._eval_model(x, t, to_x0=False)

    def data_prediction_fn(self, x, t):
        """Return the data prediction model, with corrector (ref :433-442)."""
        return self._eval_model(x, t, to_x0=True)

    def model_fn(self, x, t):
        """noise prediction for 'dpmsolver', data prediction for 'dpmsolver++' (ref :444-451)."""
        return self._eval_model(x, t, to_x0=self.algorithm_type == "dpmsolver++")

    def denoise_to_zero_fn(self, x, s):
        """ref :541-545"""
        return self.data_prediction_fn(x, s)

    # ------------------------------------------------------------------------------------------
    # time grids (ref :453-539)
    # ------------------------------------------------------------------------------------------
    def get_time_steps(self, skip_type, t_T, t_0, N, device):
        if skip_type not in L.SKIP:
            raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'".format(skip_type))
        ns = self.noise_schedule
        if skip_type == 'logSNR' and ns.schedule == 'discrete' and ns.dtype == torch.float64:
            # ref :467-471 on double tables: the fp32 logSNR grid goes through inverse_lambda, whose interpolation concatenates
            # it with the tables -- the time steps are doubles (the values the double-precision plan of sample() uses)
            lambda_T, lambda_0 = ns.marginal_lambda(torch.tensor(t_T)), ns.marginal_lambda(torch.tensor(t_0))
            return ns.inverse_lambda(torch.linspace(lambda_T.item(), lambda_0.item(), N + 1)).to(device)
        out = np.empty(N + 1, dtype=np.float32)
        L.check(L.lib.dpm_time_steps(self._h, L.SKIP[skip_type], float(t_T), float(t_0), int(N),
                                     out.ctypes.data_as(C.POINTER(C.c_float))))
        return torch.from_numpy(out).to(device)

    def get_orders_and_timesteps_for_singlestep_solver(self, steps, order, skip_type, t_T, t_0, device):
        if order not in (1, 2, 3):
            raise ValueError("'order' must be '1' or '2' or '3'.")
        if skip_type not in L.SKIP:
            raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'".format(skip_type))
        outer = np.empty(steps + 2, dtype=np.float32)
        orders = (C.c_int * (steps + 1))()
        n = C.c_int()
        L.check(L.lib.dpm_singlestep_grid(self._h, int(steps), int(order), L.SKIP[skip_type], float(t_T), float(t_0),
                                          outer.ctypes.data_as(C.POINTER(C.c_float)), orders, C.byref(n)))
        orders = [int(orders[i]) for i in range(n.value)]
        ns = self.noise_schedule
        if skip_type == 'logSNR' and ns.schedule == 'discrete' and ns.dtype == torch.float64:
            # (double time steps, see get_time_steps; ref :534-536: with 'logSNR' the outer grid is a grid of K = len(orders) steps)
            return self.get_time_steps(skip_type, t_T, t_0, len(orders), device), orders
        return torch.from_numpy(outer[: n.value + 1].copy()).to(device), orders

    # ------------------------------------------------------------------------------------------
    # public per-update methods (ref :547-954)
    # ------------------------------------------------------------------------------------------


    _exec_single = _updates.exec_single
    _singlestep_stages = _updates.singlestep_stages
    _multistep = _updates.multistep

    def dpm_solver_first_update(self, x, s, t, model_s=None, return_intermediate=False):
        """DPM-Solver-1 (equivalent to DDIM) from time `s` to time `t` (ref :547-592)."""
        stages, c64s, tf64 = self._singlestep_stages(x, 1, 0, s, t, 0., 0., 0)
        x_t, ms = self._exec_single(stages, x, {0: model_s} if model_s is not None else {}, return_intermediate, c64s, tf64, times=(s, t))
        return (x_t, {'model_s': ms[0]}) if return_intermediate else x_t

    def singlestep_dpm_solver_second_update(self, x, s, t, r1=0.5, model_s=None, return_intermediate=False,
                                            solver_type='dpmsolver'):
        """Singlestep solver DPM-Solver-2 from time `s` to time `t` (ref :594-673)."""
        if solver_type not in ['dpmsolver', 'taylor']:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        if r1 is None:
            r1 = 0.5
        mode = 1 if (torch.is_tensor(r1) and r1.dtype is not torch.float64) else 0    # (a double tensor acts like a Python float)
        stages, c64s, tf64 = self._singlestep_stages(x, 2, L.SOLVER[solver_type], s, t, r1 if mode else float(r1), 0., mode)
        # (the intermediate time s1 comes out of inverse_lambda, (1,)-shaped on a 'linear' schedule, ref :161: dimensioned --
        # and a double when the call's times are: the coefficients at s1 then promote the whole update to double)
        x_t, ms = self._exec_single(stages, x, {0: model_s} if model_s is not None else {}, return_intermediate, c64s, tf64,
                                    times=(s, t, torch.zeros(1, dtype=torch.float64 if tf64 else torch.float32)))
        return (x_t, {'model_s': ms[0], 'model_s1': ms[1]}) if return_intermediate else x_t

    def singlestep_dpm_solver_third_update(self, x, s, t, r1=1. / 3., r2=2. / 3., model_s=None, model_s1=None,
                                           return_intermediate=False, solver_type='dpmsolver'):
        """Singlestep solver DPM-Solver-3 from time `s` to time `t` (ref :675-794)."""
        if solver_type not in ['dpmsolver', 'taylor']:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        if r1 is None:
            r1 = 1. / 3.
        if r2 is None:
            r2 = 2. / 3.
        mode = 1 if any(torch.is_tensor(r) and r.dtype is not torch.float64 for r in (r1, r2)) else 0
        stages, c64s, tf64 = self._singlestep_stages(x, 3, L.SOLVER[solver_type], s, t, r1 if mode else float(r1),
                                                     r2 if mode else float(r2), mode)
        given = {}
        if model_s is not None:
            given[0] = model_s
        if model_s1 is not None:
            given[1] = model_s1
        if 1 in given and 0 not in given:
            # reference: model_s is evaluated at (x, s) even when model_s1 is supplied (ref :720-721)
            given[0] = self.model_fn(x, s)
        # the taylor combination reads model_s1 (h2): keep it even when not asked for
        x_t, ms = self._exec_single(stages, x, given, return_intermediate or solver_type == 'taylor', c64s, tf64,
                                    times=(s, t, torch.zeros(1, dtype=torch.float64 if tf64 else torch.float32)))
        return (x_t, {'model_s': ms[0], 'model_s1': ms[1], 'model_s2': ms[2]}) if return_intermediate else x_t


    def multistep_dpm_solver_second_update(self, x, model_prev_list, t_prev_list, t, solver_type="dpmsolver"):
        """Multistep solver DPM-Solver-2 from time `t_prev_list[-1]` to time `t` (ref :796-852)."""
        if solver_type not in ['dpmsolver', 'taylor']:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        return self._multistep(x, model_prev_list, t_prev_list, t, 2, solver_type)

    def multistep_dpm_solver_third_update(self, x, model_prev_list, t_prev_list, t, solver_type='dpmsolver'):
        """Multistep solver DPM-Solver-3 from time `t_prev_list[-1]` to time `t` (ref :854-904)."""
        return self._multistep(x, model_prev_list, t_prev_list, t, 3, solver_type if solver_type in L.SOLVER else 'dpmsolver')

    def singlestep_dpm_solver_update(self, x, s, t, order, return_intermediate=False, solver_type='dpmsolver',
                                     r1=None, r2=None):
        """Singlestep DPM-Solver with the order `order` from time `s` to time `t` (ref :906-930)."""
        if order == 1:
            return self.dpm_solver_first_update(x, s, t, return_intermediate=return_intermediate)
        elif order == 2:
            return self.singlestep_dpm_solver_second_update(x, s, t, return_intermediate=return_intermediate,
                                                            solver_type=solver_type, r1=r1)
        elif order == 3:
            return self.singlestep_dpm_solver_third_update(x, s, t, return_intermediate=return_intermediate,
                                                           solver_type=solver_type, r1=r1, r2=r2)
        else:
            raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    def multistep_dpm_solver_update(self, x, model_prev_list, t_prev_list, t, order, solver_type='dpmsolver'):
        """Multistep DPM-Solver with the order `order` from time `t_prev_list[-1]` to time `t` (ref :932-954)."""
        if order == 1:
            return self.dpm_solver_first_update(x, t_prev_list[-1], t, model_s=model_prev_list[-1])
        elif order == 2:
            return self.multistep_dpm_solver_second_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        elif order == 3:
            return self.multistep_dpm_solver_third_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        else:
            raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    # ------------------------------------------------------------------------------------------
    # adaptive step size (ref :956-1010): the control loop is host logic, the work is stage kernels
    # ------------------------------------------------------------------------------------------


    _adaptive_device = _adaptive.adaptive_device
    _adaptive_runs_on_device = _adaptive.runs_on_device

    def dpm_solver_adaptive(self, x, order, t_T, t_0, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5,
                            solver_type='dpmsolver'):
        """The adaptive step size solver based on singlestep DPM-Solver (ref :956-1010): the device-side controller where it
        applies, else the reference's host loop (dpm_solver_amd/adaptive.py)."""
        return _adaptive.solve(self, x, order, t_T, t_0, h_init, atol, rtol, theta, t_err, solver_type)

    # ------------------------------------------------------------------------------------------
    # add_noise / inverse / sample (ref :1012-1245)
    # ------------------------------------------------------------------------------------------
    def add_noise(self, x, t, noise=None):
        """xt = alpha_t * x + sigma_t * noise for every t; returns (t_size, batch, *shape) (ref :1012-1030)."""
        DV._require_gpu(x)
        nt = int(t.reshape(-1).shape[0])
        if noise is None:
            noise = torch.randn((nt, *x.shape), device=x.device)
        if x.dtype not in DV._DT:
            raise NotImplementedError("add_noise: dtype %s" % x.dtype)
        dbl, _ = self._double_call(x, t)
        # alpha_t / sigma_t of the reference are (nt,)-shaped tensors (ref :1023): when they are doubles -- a double t, or tables
        # declared dtype=float64 -- or x / noise is, torch's type promotion makes the result float64.  Double scalars are
        # evaluated in double at the double times; fp32 scalars meeting a double tensor are converted exactly.
        wide = dbl or x.dtype is torch.float64 or noise.dtype is torch.float64
        # (alpha_t / sigma_t are fp32 tensors of shape (nt,): half x / noise are promoted to fp32 as well)
        xdt = torch.float64 if wide else torch.promote_types(torch.promote_types(x.dtype, noise.dtype), torch.float32)
        th = t.detach().to(device="cpu", dtype=torch.float64 if dbl else torch.float32).reshape(-1).numpy().copy()
        out = DV._add_noise(self._h, x.to(xdt).contiguous(), noise.to(xdt).contiguous(), th)
        return out.squeeze(0) if nt == 1 else out

    def inverse(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform',
                method='multistep', lower_order_final=True, denoise_to_zero=False, solver_type='dpmsolver',
                atol=0.0078, rtol=0.05, return_intermediate=False):
        """Inverse the sample `x` from time `t_start` to `t_end` by DPM-Solver (ref :1032-1045)."""
        t_0 = 1. / self.noise_schedule.total_N if t_start is None else t_start
        t_T = self.noise_schedule.T if t_end is None else t_end
        assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
        return self.sample(x, steps=steps, t_start=t_0, t_end=t_T, order=order, skip_type=skip_type,
                           method=method, lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero,
                           solver_type=solver_type, atol=atol, rtol=rtol, return_intermediate=return_intermediate)


    _get_plan = _plan_cache.get_plan
    _run_plan = _loops.run_plan
    _run_plan_fast = _loops.run_plan_fast
    _run_plan_group = _loops.run_plan_group
    _auto_captured = _capture.auto_captured

    def _sample_plan(self, x, steps, t_0, t_T, order, skip_type, method, lower_order_final, denoise_to_zero, solver_type,
                     sde=False, unipc=None):
        """The plan of a multistep / singlestep / singlestep_fixed `sample()` call, with the reference's argument checks and
        errors (shared by sample() and the request pool)."""
        if method == 'multistep':
            assert steps >= order                       # (the reference's first check, ref :1172)
        elif method == 'singlestep' and order not in (1, 2, 3):
            raise ValueError("'order' must be '1' or '2' or '3'.")    # ref :533, before the grid is built
        elif method == 'singlestep_fixed':
            steps // order                              # ref :1218: K = steps // order (ZeroDivisionError for order 0)
        if skip_type not in L.SKIP:
            raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'".format(skip_type))
        plan_solver_type = solver_type
        if solver_type not in L.SOLVER:
            # the reference checks solver_type inside its second-order updates and the singlestep third-order one (ref
            # :611, :697, :815), i.e. only when such an update is reached: a run made of first-order (and multistep
            # third-order) updates accepts any value.  Plan with the default to see which updates the run contains.
            plan_solver_type = "dpmsolver"
        if method == 'multistep':
            # the order is validated where the reference validates it -- when an update of that order is reached
            # (ref :948-954): order=4 with steps <= 6 and lower_order_final never reaches one and runs (the planner
            # raises the reference's ValueError otherwise)
            assert steps >= order
            if order > 3 and plan_solver_type is not solver_type:
                # ... and the warm-up of such a run passes through a second-order update first (ref :1185-1193)
                raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        elif method == 'singlestep_fixed' and order not in (1, 2, 3):
            # ref :1218-1232: K = steps // order updates of that order -- none at all when K <= 0 (the run is a no-op),
            # else the dispatcher's error at the first one (ref :927-930); order 0 is Python's ZeroDivisionError
            K = steps // order
            if K > 0:
                raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))
            order, steps = 3, 1                    # a plan without update stages (K = 1 // 3 = 0)
        elif order not in (1, 2, 3):
            raise ValueError("'order' must be '1' or '2' or '3'.")
        plan = self._get_plan(precision=self._precision(self._sdtype(x)), method=method, order=order, steps=steps,
                              skip_type=skip_type, solver_type=plan_solver_type,
                              lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero,
                              t_T=float(t_T), t_0=float(t_0), **({"sde": True} if sde else {}),
                              **({"unipc": unipc} if unipc else {}))
        if plan_solver_type is not solver_type and any(st.form in (L.FORM_TWO, L.FORM_SS3T) for st in plan.stages):
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        return plan

    def sample(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform',
               method='multistep', lower_order_final=True, denoise_to_zero=False, solver_type='dpmsolver',
               atol=0.0078, rtol=0.05, return_intermediate=False):
        """Compute the sample at time `t_end` by DPM-Solver, given the initial `x` at time `t_start`
        (signature and semantics of ref :1047-1245; see that docstring for the argument meanings)."""
        t_0 = 1. / self.noise_schedule.total_N if t_end is None else t_end
        t_T = self.noise_schedule.T if t_start is None else t_start
        assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
        if return_intermediate:
            assert method in ['multistep', 'singlestep', 'singlestep_fixed'], "Cannot use adaptive solver when saving intermediate values"
        if self.correcting_xt_fn is not None:
            assert method in ['multistep', 'singlestep', 'singlestep_fixed'], "Cannot use adaptive solver when correcting_xt_fn is not None"
        DV._require_gpu(x)
        device = x.device
        intermediates = []
        cxt = self.correcting_xt_fn
        if self.auto_capture and self._group is None and not torch.cuda.is_current_stream_capturing():
            hit = self._auto_captured(x, dict(steps=steps, t_start=t_start, t_end=t_end, order=order, skip_type=skip_type,
                                              method=method, lower_order_final=lower_order_final,
                                              denoise_to_zero=denoise_to_zero, solver_type=solver_type, atol=atol, rtol=rtol),
                                      return_intermediate)
            if hit is not None:
                return hit
        with torch.no_grad():
            if method == 'adaptive':
                x = self.dpm_solver_adaptive(x, order=order, t_T=t_T, t_0=t_0, atol=atol, rtol=rtol, solver_type=solver_type)
                if denoise_to_zero:
                    x = self.denoise_to_zero_fn(x, self._tt(t_0, device, shape1=True))
            elif method in ['multistep', 'singlestep', 'singlestep_fixed']:
                plan = self._sample_plan(x, steps, t_0, t_T, order, skip_type, method, lower_order_final, denoise_to_zero,
                                         solver_type)
                x = self._run_plan(plan, x, method, cxt, return_intermediate, intermediates)
            else:
                raise ValueError("Got wrong method {}".format(method))
        if return_intermediate:
            return x, intermediates
        else:
            return x

    sample_sde = _sde.sample_sde
    sample_sde_requests = _sde.sample_sde_requests
    sample_unipc = _unipc.sample_unipc
    sample_unipc_requests = _unipc.sample_unipc_requests

    def sample_requests(self, xs, **sample_kwargs):
        """(extension) `sample()` for several independent requests that are in flight together -- a server's batch of
        sampling jobs with their own states, e.g. `xs = [x_T_0, ..., x_T_31]`, all of one shape, dtype and device.
        Returns the list of results, identical to `[sample(x, **sample_kwargs) for x in xs]`.

        The requests are advanced stage by stage: the network is called once per request (each on its own state), then
        ONE fused kernel advances all of them (dpm_stage_launch_multi; 32 requests per launch).  A lone 42 MB launch
        whose inputs come from HBM -- they always do when a network ran in between -- spends a third of its time ramping
        up and draining; fused, that is paid once per stage instead of once per request (8.5 -> 6.6 us per
        `[256,4,64,64]` fp16 request-stage), and thresholded stages of small batches stop needing workgroup clusters
        (11.4 -> 1.4 us per request-stage for 32 requests of `[32,3,64,64]`).  Calls with correctors written in Python,
        `return_intermediate` or the adaptive method run the requests one after the other."""
        xs = list(xs)
        kw = sample_kwargs
        ok = (len(xs) > 1 and kw.get("method", "multistep") in ("multistep", "singlestep", "singlestep_fixed")
              and not kw.get("return_intermediate", False) and self.correcting_xt_fn is None and self._user_x0 is None
              and all(torch.is_tensor(x) and x.shape == xs[0].shape and x.dtype == xs[0].dtype and x.device == xs[0].device
                      for x in xs) and xs[0].dim() > 0 and xs[0].numel() > 0)
        if not ok:
            return [self.sample(x, **kw) for x in xs]
        self._group = xs
        try:
            return self.sample(xs[0], **kw)      # _run_plan picks the group up and returns the list of results
        finally:
            self._group = None


    def request_pool(self, mixed_shapes=False, slots=None, sde=False, thresholding=False, inpaint=False, rescale=False,
                     apg=False, zero_star=False, pair=False, perp_neg=False):
        """(extension) A pool of sampling requests for continuous batching: requests are submitted at any time with their
        own `sample()` arguments, every `step()` advances each active request by one stage -- the network once per request,
        then one fused launch for all of them whatever their positions -- and returns the finished ones.  Results are
        bit-identical to `sample()`; see dpm_solver_amd/pool.py.  `mixed_shapes=True`: the requests may differ in shape (latent
        size, images per prompt) and still share the tick's launch.
        `slots=S`: a `SlabPool` (dpm_solver_amd/slab.py) for MANY SMALL requests -- S rows of one sample each in slabs the
        pool owns; a tick is one network call on the whole slab, one host-to-device copy and one table-driven stage launch
        (dpm_launch_opts.table_mode), and every request may bring its own condition.  `slots=S, sde=True`: the slab pool
        also admits SDE-DPM-Solver++ requests (`submit(x, ..., sde=True, seed=...)`), their stages in the table-driven launch
        too (DPM_TABLE_NOISE).  `slots=S, thresholding=True`: the slab pool of a solver built with
        correcting_x0_fn="dynamic_thresholding" -- samples of at most 12288 elements, their thresholded stages in the
        table-driven launch too (DPM_TABLE_THRESH); without the flag a slab pool refuses such a solver.
        `slots=S, inpaint=True` (alone or with sde=True): the slab pool also admits inpainting / DiffEdit requests
        (`submit(x, ..., blend=MaskBlend(...))`, the result of sample() with correcting_xt_fn=blend), their mask-blend stages
        in the table-driven launch too (DPM_TABLE_BLEND).
        `slots=S, rescale=True`: the slab pool of a classifier-free wrapper that admits guidance-rescale requests -- the
        wrapper's own phi (`cfg_rescale`) or the request's (`submit(x, ..., guidance_rescale=phi)`), their stages in the
        table-driven launch too (DPM_TABLE_RESCALE: one stage_rescale_kernel_table launch, one workgroup per row); samples of
        whole 8-element groups.  Not together with sde / thresholding / inpaint (the rescale kernel has none of those
        epilogues); without the flag a slab pool refuses a `cfg_rescale` solver.
        `slots=S, apg=True`: the slab pool of a classifier-free wrapper that admits adaptive-projected-guidance requests --
        the wrapper's own parameters (`cfg_apg`) or the request's (`submit(x, ..., apg=(eta, norm_threshold, momentum))`),
        their stages in the table-driven launch too (DPM_TABLE_APG: one stage_apg_kernel_table launch, one workgroup per row;
        the pool holds the running averages in a slab of its own, zeroed at admission); samples of whole 8-element groups, a
        data-prediction solver.  Not together with rescale / sde / thresholding / inpaint (the APG kernel has none of those
        epilogues); without the flag a slab pool refuses a `cfg_apg` solver.
        `slots=S, zero_star=True`: the slab pool of a classifier-free wrapper that admits CFG-Zero* requests -- the wrapper's
        own setting (`cfg_zero_star`) or the request's (`submit(x, ..., zero_star=True | False)`), their stages in the
        table-driven launch too (DPM_TABLE_ZSTAR: one stage_zstar_kernel_table launch, one workgroup per row; no record, no
        state); samples of whole 8-element groups.  Not together with rescale / apg / sde / thresholding / inpaint (the
        CFG-Zero* kernel has none of those epilogues); without the flag a slab pool refuses a `cfg_zero_star` solver.
        `slots=S, pair=True`: the slab pool of a `cfg_pair` wrapper (guidance over two conditions): slabs of [3S, ...] in the
        wrapper's order (unconditional, condition, condition2), every request with its own conditions and two scales
        (`submit(x, ..., condition2=c2, guidance_scale=s, pair=(scale2, nested))`), their stages in the table-driven launch
        (DPM_TABLE_PAIR: one stage_pair_kernel_table launch that stores the result three times -- no `torch.cat([x] * 3)`);
        samples of whole 8-element groups.  Not together with sde / thresholding / inpaint / rescale / apg / zero_star;
        without the flag a pool refuses a `cfg_pair` solver.  `pair=True` refuses a `cfg_perp_neg` solver (its rows have no
        per-sample pass): that solver's slab pool is `perp_neg=True`, below; a RequestPool (no slots) takes it as it is, each of
        its stages a launch of its own inside the tick's call.
        `slots=S, perp_neg=True`: the slab pool of a `cfg_perp_neg` wrapper (Perp-Neg): slabs of [3S, ...] in the wrapper's
        order (empty prompt, positive, negative), every request with its own three conditions and two scales
        (`submit(x, ..., negative_condition=n, guidance_scale=s, neg_scale=w)`, either scale without the other), their stages
        in the table-driven launch (DPM_TABLE_PERP: one stage_perp_kernel_table launch, one workgroup per sample, that stores
        the result three times -- no `torch.cat([x] * 3)`); samples of whole 8-element groups.  Not together with sde /
        thresholding / inpaint / rescale / apg / zero_star / pair; without the flag a slab pool refuses a `cfg_perp_neg` solver.
        Every classifier-free slab pool takes a guidance scale per request: `submit(x, ..., guidance_scale=g)`."""
        if sde and slots is None:
            raise ValueError("request_pool: sde=True belongs to a slab pool (slots=...); a RequestPool takes sde per submit")
        if thresholding and slots is None:
            raise ValueError("request_pool: thresholding=True belongs to a slab pool (slots=...); a RequestPool takes a "
                             "thresholding solver as it is")
        if inpaint and slots is None:
            raise ValueError("request_pool: inpaint=True belongs to a slab pool (slots=...); a RequestPool takes no "
                             "correcting_xt_fn")
        if inpaint and thresholding:
            raise NotImplementedError("request_pool: inpaint=True with thresholding=True -- the thresholded table rows have "
                                      "no mask blend")
        if perp_neg:
            if slots is None:
                raise ValueError("request_pool: perp_neg=True belongs to a slab pool (slots=...)")
            if not self._perp():
                raise ValueError("request_pool: perp_neg=True needs a cfg_perp_neg wrapper (Perp-Neg guidance with a negative "
                                 "scale other than 0)")
            for name, why in (("sde", "no noise epilogue"), ("thresholding", "no thresholding"),
                              ("inpaint", "no mask-blend epilogue"), ("rescale", "no guidance rescale"),
                              ("apg", "no projected guidance"), ("zero_star", "no CFG-Zero* projection"),
                              ("pair", "no linear second blend")):
                if dict(sde=sde, thresholding=thresholding, inpaint=inpaint, rescale=rescale, apg=apg, zero_star=zero_star,
                        pair=pair)[name]:
                    raise NotImplementedError("request_pool: perp_neg=True with %s=True -- the Perp-Neg kernel has %s (a "
                                              "follow-up)" % (name, why))
            self._check_pair()
        elif pair:
            if slots is None:
                raise ValueError("request_pool: pair=True belongs to a slab pool (slots=...)")
            if self._perp():
                raise NotImplementedError("request_pool: pair=True with a cfg_perp_neg wrapper -- the table's two-condition rows "
                                          "have no per-sample pass (a follow-up)")
            if self._pair_setting() is None:
                raise ValueError("request_pool: pair=True needs a cfg_pair wrapper (guidance over two conditions with a second "
                                 "scale other than 0)")
            for name, why in (("sde", "no noise epilogue"), ("thresholding", "no thresholding"),
                              ("inpaint", "no mask-blend epilogue"), ("rescale", "no guidance rescale"),
                              ("apg", "no projected guidance"), ("zero_star", "no CFG-Zero* projection")):
                if dict(sde=sde, thresholding=thresholding, inpaint=inpaint, rescale=rescale, apg=apg, zero_star=zero_star)[name]:
                    raise NotImplementedError("request_pool: pair=True with %s=True -- the two-condition kernel has %s (a "
                                              "follow-up)" % (name, why))
            self._check_pair()
        elif self._perp() and slots is None:
            self._check_pair()      # a RequestPool takes a cfg_perp_neg solver as it is: such a stage runs on its own in a tick's launch
        else:
            self._check_pair("request_pool -- a pool's ticks are fused and table-driven launches, and a two-condition stage runs "
                             "on its own in those (sample_requests takes such a solver; request_pool(slots=..., pair=True) is its "
                             "slab pool)")
        on = dict(sde=sde, thresholding=thresholding, inpaint=inpaint, rescale=rescale, apg=apg, zero_star=zero_star)
        _rem.check_switches(self, slots, on)
        if thresholding and not self._thresholding:
            raise ValueError("request_pool: thresholding=True on a solver built without "
                             "correcting_x0_fn='dynamic_thresholding'")
        if slots is not None:
            _rem.check_slab(self, on)
            if mixed_shapes:
                raise ValueError("request_pool: a slab pool (slots=...) holds rows of one sample shape; mixed_shapes is the "
                                 "RequestPool's")
            return _slab.SlabPool(self, slots, sde=sde, thresholding=thresholding, inpaint=inpaint, rescale=rescale, apg=apg,
                                  zero_star=zero_star, pair=pair, perp_neg=perp_neg)
        return _pool.RequestPool(self, mixed_shapes=mixed_shapes)

    def capture(self, x, warmup=2, **sample_kwargs):
        """hipGraph-capture `sample(x, **sample_kwargs)` for a fixed shape (extension).

        The step loop is launch-bound between network calls -- a stage kernel runs for microseconds -- so the whole
        trajectory (network calls included) is recorded once into a HIP graph and replayed with one launch:

            g = dpm_solver.capture(x_T, steps=20, order=2)     # warm-up runs + capture (on a side stream)
            out = g(x_T_new)                                    # copy into the static input, replay

        Requirements are those of torch.cuda.graph: the wrapped network must be capturable (no host
        synchronisation, no data-dependent control flow), shapes are frozen, and the returned tensors are static
        buffers that the next replay overwrites.  method='adaptive' is captured with its device-side controller: exactly
        `adaptive_max_iterations` (default 64) iterations are recorded, those after t_end is reached do nothing."""
        self._check_pair()
        apg = self._remedy_setting("cfg_apg")
        if apg is not None and apg[2] != 0.0:
            self._check_remedies("capture with a momentum -- a replayed graph would carry the running average of one run into "
                                 "the next; capture with momentum=0, or sample() eagerly", only="cfg_apg")
        if sample_kwargs.get("method", "multistep") == "adaptive" and not self._adaptive_runs_on_device(x):
            raise NotImplementedError("the host-side adaptive control loop synchronises every iteration; it cannot be "
                                      "captured into a graph (the device-side controller can: adaptive_on_device = True, no "
                                      "dynamic thresholding / callable correcting_x0_fn, an fp32 or explicit half state)")
        return GraphedSample(self, x, warmup, sample_kwargs)


# ---------------------------------------------------------------------------------------------------------------------
# Compatibility: until round 6 the device entry points were attributes of THIS module, and the CPU test suite
# (tests/kernel_double.py: install_cpu_double), the GPU launch spies and tools/ hook in by assigning to them --
# `solver._stage_launch_raw = shim`, `monkeypatch.setattr(solver, "_launch_stage", double)`.  They live in _device.py now,
# and every module calls them as `DV.<name>`; reads and writes of those names on this module are forwarded there.
# ---------------------------------------------------------------------------------------------------------------------
class _SolverModule(types.ModuleType):
    def __getattr__(self, name):                  # only reached for names this module does not define itself
        try:
            return getattr(DV, name)
        except AttributeError:
            raise AttributeError("module %r has no attribute %r" % (self.__name__, name)) from None

    def __setattr__(self, name, value):
        if name not in self.__dict__ and hasattr(DV, name):
            setattr(DV, name, value)
        else:
            super().__setattr__(name, value)

    def __delattr__(self, name):
        if name not in self.__dict__ and hasattr(DV, name):
            delattr(DV, name)
        else:
            super().__delattr__(name)


sys.modules[__name__].__class__ = _SolverModule
