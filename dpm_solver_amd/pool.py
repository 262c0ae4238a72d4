"""Continuous batching: a pool of sampling requests that arrive, advance and finish independently (`DPM_Solver.request_pool()`).

`sample_requests` advances requests in lockstep -- one plan, one position.  A server's requests arrive while others are
mid-trajectory and ask for their own step counts and orders; the pool takes them whenever they come:

    pool = dpm_solver.request_pool()
    h = pool.submit(x_T, steps=20, order=2)         # any time between ticks
    done = pool.step()                              # one stage of every active request -> {handle: result} of those finished
    while pool:
        done.update(pool.step())

One tick calls the network once per active request, on its own state at its own stage, and advances all of them with ONE
dpm_stage_launch_multi whose stage records are per request (dpm_launch_opts.per_request_stages): the library fuses the
requests its heterogeneous kernel covers and launches the rest one by one.  Every result is bit-identical to
`sample(x_T, **its kwargs)`, whatever else was in flight.

`submit(..., sde=True, seed=...)` admits an SDE-DPM-Solver++ request (`sample_sde`'s arguments and checks): its seed is
resolved at submission and travels in a dpm_launch_opts of the request's own, pointed to by its dpm_buffers entry of every
tick -- never by the launch records, which finished requests hand on to later ones.  The library fuses SDE stages in groups
of their own, next to the ODE groups of the same tick; the result is bit-identical to `sample_sde(x_T, seed=..., ...)`.

`submit_unipc(x_T, steps=20, order=2, variant='bh2', ...)` admits a UniPC request (`sample_unipc`'s arguments and checks, minus
`return_intermediate`).  Its plan is a first-order stage followed by DPM_FORM_UNIPC stages, which the heterogeneous launch
fuses at any position next to the first- and second-order stages of other requests (stage_kernel_het_unipc), so a pool of
UniPC requests -- or of UniPC and 2M requests -- is one launch per tick and 16 requests; the result is bit-identical to
`sample_unipc(x_T, ...)`.  One pool may hold ODE, SDE and UniPC requests at once.

`request_pool(mixed_shapes=True)` admits requests of ANY shape -- 512^2, 768^2 and 1024^2 latents, different images per prompt
-- into one pool; dtype and device stay the first submit's.  The tick's options then carry dpm_launch_opts.fuse_shapes, and
the library fuses requests of different element counts in one launch of its mixed-shape kernels (stage_kernel_shapes: the
members' tiles back to back, each request advanced over its own size), 16 requests per launch as before.  A request the fused
kernels do not take (an element count that is no multiple of 8, for one) is launched on its own in the same call.  Results
stay bit-identical to `sample` / `sample_sde` / `sample_unipc` on the request alone.  The default pool fixes the shape at the
first submit and launches exactly as it did before the flag existed.
"""
import ctypes as C

import torch

from . import _device as DV
from . import _lib as L
from . import sde as _sde
from . import unipc as _unipc
from .launch_list import _FastRun, _bind_outputs
from .plan_cache import _Cloning

_METHODS = ("multistep", "singlestep", "singlestep_fixed")


class _Request:
    """one request in flight: its plan, its launch records (a _FastRun of its own) and its position"""
    __slots__ = ("x", "plan", "i", "V", "sd", "mf", "fr", "key", "x0", "out", "first", "seed", "opts")


class RequestPool:
    """Requests of one shape, dtype and device (fixed by the first submit), each with its own `sample()` arguments.
    `mixed_shapes=True`: of one dtype and device, any shape."""

    def __init__(self, solver, mixed_shapes=False):
        self._s = solver
        self._mixed = bool(mixed_shapes)
        self._active = {}        # handle -> _Request, in submission order
        self._finished = {}      # handle -> result of a request without update stages (returned by the next step)
        self._free = {}          # launch-record key -> [_FastRun]: scratch of finished requests, reused by later ones
        self._next = 0
        self._like = None        # (shape, dtype, device) of the pool; a mixed-shape pool: (None, dtype, device)
        self._opts = L.LaunchOpts()

    def __len__(self):
        return len(self._active) + len(self._finished)

    def __bool__(self):
        return len(self) > 0

    def submit(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', method='multistep',
               lower_order_final=True, denoise_to_zero=False, solver_type='dpmsolver', return_intermediate=False,
               sde=False, seed=None, generator=None, unipc=None):
        """Admit a request: `x` = its x_T, the rest as for `sample()` (multistep, singlestep and singlestep_fixed methods),
        validated with sample()'s errors.  `sde=True`: an SDE-DPM-Solver++ request -- `sample_sde`'s arguments, checks and
        seed rules (`seed`, or one draw from `generator` / torch's default CPU generator, made here).  Returns the request's
        handle (an int)."""
        s = self._s
        if unipc:
            raise NotImplementedError("request pool: submit() takes sample()'s arguments; admit a UniPC request with "
                                      "submit_unipc(x, steps=..., order=..., variant=...)")
        if not sde and (seed is not None or generator is not None):
            raise ValueError("request pool: `seed` / `generator` belong to an SDE request (sde=True)")
        if sde:
            if method != 'multistep':
                raise ValueError("request pool: sde=True samples by the multistep SDE-DPM-Solver++ (method='multistep'), "
                                 "got method={!r}".format(method))
            _sde.check_solver(s, order)
            seed = _sde.resolve_seed(seed, generator)
            if torch.is_tensor(x):
                _sde.check_state(s, x)
        if method == 'adaptive':
            raise NotImplementedError("request pool: method='adaptive' has no plan of stages (its step sizes depend on the "
                                      "state); sample it with sample()")
        if return_intermediate:
            raise NotImplementedError("request pool: return_intermediate is not supported; sample it with sample()")
        if s.correcting_xt_fn is not None:
            raise NotImplementedError("request pool: a correcting_xt_fn runs Python between stages; sample with sample()")
        if s._user_x0 is not None:
            raise NotImplementedError("request pool: a callable correcting_x0_fn runs Python between stages; sample with "
                                      "sample()")
        if method not in _METHODS:
            raise ValueError("Got wrong method {}".format(method))
        like = self._check_x(x)
        t_0 = 1. / s.noise_schedule.total_N if t_end is None else t_end
        t_T = s.noise_schedule.T if t_start is None else t_start
        assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
        with torch.no_grad():
            plan = s._sample_plan(x, steps, t_0, t_T, order, skip_type, method, lower_order_final, denoise_to_zero,
                                  solver_type, sde=bool(sde))
        return self._admit(x, like, plan, seed if sde else None)

    def submit_unipc(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', variant='bh2',
                     corrector=True, lower_order_final=True, denoise_to_zero=False):
        """Admit a UniPC request: `x` = its x_T, the rest as for `sample_unipc()` (no `return_intermediate`), validated with
        sample_unipc()'s errors in its order, then the pool's own (the device requirement, a non-tensor, a shape / dtype /
        device other than the pool's) -- all before any device work.  `corrector=False` (variant 'bh2') admits sample()'s
        multistep DPM-Solver++ plan, as sample_unipc runs it.  Returns the request's handle."""
        s = self._s
        _unipc.check_solver(s, order, variant)
        t_0, t_T = _unipc._times(s, t_start, t_end)
        if not torch.is_tensor(x):
            self._check_x(x)          # (check_state and the planner read x.dtype: a non-tensor gets the pool's error here)
        _unipc.check_state(s, x)
        if not corrector:
            if variant != 'bh2':
                raise NotImplementedError("sample_unipc: corrector=False with variant='bh1' (the predictor alone is built for "
                                          "'bh2', where it is DPM-Solver++ 2M)")
            return self.submit(x, steps=steps, t_start=t_start, t_end=t_end, order=order, skip_type=skip_type,
                               method='multistep', lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero,
                               solver_type='dpmsolver')
        with torch.no_grad():
            plan = s._sample_plan(x, steps, t_0, t_T, order, skip_type, 'multistep', lower_order_final, denoise_to_zero,
                                  'dpmsolver', unipc=variant)
        return self._admit(x, self._check_x(x), plan, None)

    def _check_x(self, x):
        """the pool's own checks of a request's x_T: on the GPU, a tensor of the pool's shape (unless it mixes shapes), dtype
        and device; returns what _admit stores as the pool's (shape, dtype, device)"""
        DV._require_gpu(x)
        if not torch.is_tensor(x) or x.dim() == 0 or x.numel() == 0:
            raise ValueError("request pool: x must be a tensor with at least one dimension and one element")
        like = (tuple(x.shape), x.dtype, x.device)
        if self._like is not None and like[1 if self._mixed else 0:] != self._like[1 if self._mixed else 0:]:
            raise ValueError("request pool: x of shape %s, dtype %s on %s does not match the pool's %s, %s on %s"
                             % (like + (self._like[0] or "any shape",) + self._like[1:]))
        return ((None,) + like[1:]) if self._mixed else like

    def _admit(self, x, like, plan, seed):
        """a checked request with its plan joins the pool (seed: an SDE request's); returns its handle"""
        s = self._s
        sd = s._sdtype(x)
        s._check_remedies(sd=sd)            # (a pool's requests do not pass run_plan)
        if s._perp():
            s._check_pair()                 # (cfg_perp_neg: taken as it is -- each of its stages a launch of its own in the tick's call)
        else:
            s._check_pair("request_pool -- a pool's ticks are fused launches, and a two-condition stage runs on its own in those")
        if (s._state_dtype is None and sd not in (torch.float32, torch.float64) and plan.stages
                and plan.stages[-1].form == L.FORM_DENOISE and s.noise_schedule.schedule != 'discrete'):
            raise NotImplementedError("request pool: denoise_to_zero with a half-precision state on a continuous schedule "
                                      "ends in an fp32 stage outside the fast path; sample it with sample()")
        self._like = like
        h = self._next
        self._next += 1
        if not plan.stages:       # singlestep_fixed with steps < order: no update at all, x comes back as it is
            self._finished[h] = x
            return h
        q = _Request()
        q.x, q.plan, q.i, q.sd = x, plan, 0, sd
        q.seed = seed
        q.opts = L.LaunchOpts() if seed is not None else None      # its own options: the solver's + its seed (step)
        self._active[h] = q
        return h

    def _start(self, q, cfg, stream, idx):
        """the first stage of a request: its network output on the caller's x_T decides the state dtype and layout"""
        s = self._s
        q.V = s._time_views(q.plan, q.x.device, q.x.shape[0], cfg)
        q.first = self._net(q, q.x, 0, None, cfg)
        q.sd = s._promoted(q.sd, q.first[0], q.plan)
        q.mf = DV._mf_of(q.first[0]) if q.first[0].shape == q.x.shape else None
        if q.plan.sde:
            q.mf = None    # the noise contract indexes the default [B, C, H, W] order (include/dpm_hip.h): contiguous states
        q.key = (id(q.plan), tuple(q.x.shape), q.sd, idx, stream, cfg, q.mf, bool(s.cluster_in_graph), int(s.thr_spin_limit),
                 s._remedy_key(), s._pair_key())
        free = self._free.get(q.key)
        q.fr = free.pop() if free else _FastRun(s, q.plan, q.x.shape, q.sd, q.x.device, cfg, q.mf)
        if q.fr.apg_avg is not None:
            q.fr.apg_avg.zero_()            # a request starts: its running average is zero, whoever used the records before
        q.x0 = DV._conv(q.x, q.sd, q.mf)
        q.out = DV._empty(q.x.shape, q.sd, q.x.device, q.mf)

    def _net(self, q, x_t, i, x2, cfg):
        s = self._s
        V = q.V
        tb, ti, t2 = V["t_eval_b"], V["t_input_b"], V["t_input_2b"]
        if s.fresh_time_tensors:
            tb, ti, t2 = _Cloning(tb), _Cloning(ti), (_Cloning(t2) if cfg else None)
        if s._wrapped is not None:
            e = s._wrapped.raw_outputs(x_t, tb[i], ti[i], t2[i] if cfg else None, x_in2=x2)
        else:
            e = (s._model_fn(x_t, tb[i]), None, None)
        if not s.fresh_time_tensors and q.plan.written(V):
            # the network edits its time argument in place and requests share the rows of a plan: clones from here on
            s.fresh_time_tensors = True
        return e

    def step(self):
        """One stage of every active request (network calls, then one multi-request launch).  Returns {handle: result}
        of the requests that finished: fresh tensors in the layout of their x_T."""
        done, self._finished = self._finished, {}
        if not self._active:
            return done
        s = self._s
        cfg = s._wrapped is not None and s._wrapped.effective_guidance == "classifier-free"
        device = self._like[2]
        stream, idx, capturing, other = DV._launch_ctx(device)
        if capturing:
            raise RuntimeError("request pool: ticks are not captured into graphs")
        R = len(self._active)
        sts, bufs = (L.Stage * R)(), (L.Buffers * R)()
        keep = []
        with torch.no_grad():
            for r, q in enumerate(self._active.values()):
                if q.i == 0:
                    self._start(q, cfg, stream, idx)
                fr, i = q.fr, q.i
                b = fr.bufs[i]
                xi, xei, _ = q.plan.roles[i]
                p0 = q.x0.data_ptr()
                if xi == 0:
                    b.x = p0
                if xei == 0:
                    xe_t, x2 = q.x0, None
                    if xi != 0:
                        b.xe = p0
                else:
                    xe_t, x2 = fr.xbuf[xei], (fr.xfull[xei] if cfg else None)
                if i == fr.last:
                    b.x_out = q.out.data_ptr()
                e = q.first if i == 0 else self._net(q, xe_t, i, x2, cfg)
                q.first = None
                if q.sd is torch.float64:
                    e = s._cfg_pre(e, q.sd)
                keep.append(_bind_outputs(b, e[0], e[1], e[2], q.sd, q.x.shape, q.mf, s._pair_setting() is not None))
                C.memmove(C.byref(sts, r * C.sizeof(L.Stage)), C.byref(fr.stages[i]), C.sizeof(L.Stage))
                C.memmove(C.byref(bufs, r * C.sizeof(L.Buffers)), C.byref(b), C.sizeof(L.Buffers))
        # request 0's options carry the per-request flag (the library reads bs[0].opts); an SDE request's carry its seed,
        # each in a dpm_launch_opts of its own; the others keep the solver's.  The seeds live in this tick's array only.
        o = s._opts_ptr()
        if o is not None:
            C.memmove(C.byref(self._opts), o, C.sizeof(L.LaunchOpts))
        self._opts.per_request_stages = 1
        self._opts.fuse_shapes = 1 if self._mixed else 0
        self._opts.noise_seed_lo = self._opts.noise_seed_hi = 0
        for r, q in enumerate(self._active.values()):
            if q.seed is None:
                continue
            if r == 0:
                self._opts.noise_seed_lo, self._opts.noise_seed_hi = q.seed & 0xffffffff, q.seed >> 32
            else:
                q.opts = _sde.request_opts(q.seed, o)
                bufs[r].opts = C.pointer(q.opts)
        bufs[0].opts = C.pointer(self._opts)
        if other:
            with torch.cuda.device(idx):
                rc = DV._stage_launch_multi_raw(sts, bufs, R, stream)
        else:
            rc = DV._stage_launch_multi_raw(sts, bufs, R, stream)
        self._opts.noise_seed_lo = self._opts.noise_seed_hi = 0
        if rc:
            L.check(rc)
        del keep
        for h in list(self._active):
            q = self._active[h]
            q.i += 1
            if q.i == len(q.plan.stages):
                del self._active[h]
                self._free.setdefault(q.key, []).append(q.fr)
                x = q.x
                done[h] = q.out if (q.mf is None and x.is_contiguous()) else DV._in_layout_of(q.out, x)
        return done
