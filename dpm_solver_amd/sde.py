"""SDE-DPM-Solver++ sampling: `DPM_Solver.sample_sde` (extension; "DPM++ 2M SDE", diffusers' `sde-dpmsolver++`).

The plan is `sample(method='multistep')`'s plan -- same stages, forms, times, buffer roles and history slots -- with the
stochastic update's scalars (dpm_plan_create with DPM_ALGO_SDE_DPMSOLVERPP): every first- / second-order stage adds
sigma_t * sqrt(1 - e^{-2h}) * z, z generated INSIDE the stage kernel by a counter-based generator (Philox4x32-10 keyed by the
seed, counter = element index and stage index: include/dpm_hip.h, "noise contract").  No noise tensor is written or read and
no launch is added: an SDE stage moves the bytes of the ODE stage.  The seed travels per call in dpm_launch_opts, so the
prebuilt launch records (_FastRun) and the plan cache never hold it, and the call bypasses auto_capture (a replayed graph
would bake one seed in).

Several requests (`sample_sde_requests`, `RequestPool.submit(sde=True)`): every request has a dpm_launch_opts of its own with
its seed (`request_opts`), pointed to by its entry of the dpm_buffers array for the length of one multi-request launch; the
library fuses the requests' SDE stages into one launch and keys each request's generator with its own seed.  The records
that outlive the call -- the cached groups of _FastRun, the pool's free lists -- keep the solver's seedless options.
"""
import ctypes as C

import torch

from . import _device as DV
from . import _lib as L

_U64 = 1 << 64


def resolve_seed(seed, generator):
    """the 64-bit seed of a call: `seed` as given, else one torch.randint on `generator`, else on torch's default CPU generator
    (so that torch.manual_seed(k) reproduces a run)"""
    if seed is not None and generator is not None:
        raise ValueError("sample_sde: pass either `seed` or `generator`, not both")
    if seed is not None:
        if isinstance(seed, bool) or not isinstance(seed, int) and not (torch.is_tensor(seed) and seed.numel() == 1
                                                                          and not seed.is_floating_point()):
            raise ValueError("sample_sde: `seed` must be an int in [0, 2**64), got %r" % (seed,))
        seed = int(seed)
        if not 0 <= seed < _U64:
            raise ValueError("sample_sde: `seed` must be in [0, 2**64), got %d" % seed)
        return seed
    kw = {} if generator is None else dict(generator=generator, device=generator.device)
    return int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64, **kw).item()) % _U64


def check_solver(self, order):
    """sample_sde's errors about the solver and the order (shared with sample_sde_requests and the request pool)"""
    if self.algorithm_type != "dpmsolver++":
        raise NotImplementedError("sample_sde: algorithm_type='dpmsolver' (the noise-prediction SDE variant) is not built; "
                                  "use algorithm_type='dpmsolver++'")
    self._check_remedies("sample_sde -- the SDE stage kernels have no {noun} (a follow-up)")
    self._check_pair("sample_sde -- the SDE stage kernels blend two network outputs, not three (a follow-up)")
    if self._thresholding:
        raise NotImplementedError("sample_sde: correcting_x0_fn='dynamic_thresholding' -- the thresholding kernel has no noise "
                                  "epilogue")
    if self._user_x0 is not None:
        raise NotImplementedError("sample_sde: a callable correcting_x0_fn (the stage would be split around it; the SDE "
                                  "stages have no such split)")
    if order not in (1, 2):
        raise ValueError("sample_sde: 'order' must be 1 or 2 (no third-order SDE update is defined), got {}".format(order))


def check_state(self, x):
    if self._sdtype(x) is torch.float64:
        raise NotImplementedError("sample_sde: double-precision states (there is no double noise kernel)")


def request_opts(seed, base):
    """a dpm_launch_opts of one request's own: `base` (a pointer to the solver's seedless options, or None) + its seed"""
    o = L.LaunchOpts()
    if base is not None:
        C.memmove(C.byref(o), base, C.sizeof(L.LaunchOpts))
    o.noise_seed_lo, o.noise_seed_hi = seed & 0xffffffff, seed >> 32
    return o


def sample_sde(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', lower_order_final=True,
               denoise_to_zero=False, solver_type='dpmsolver', seed=None, generator=None, return_intermediate=False):
    """Sample by SDE-DPM-Solver++ (multistep, order 1 or 2) from x_T at `t_start` to `t_end`.  `steps`, `t_start`, `t_end`,
    `skip_type`, `lower_order_final`, `denoise_to_zero` mean what they mean for `sample(method='multistep')`;
    solver_type 'dpmsolver' is diffusers' "midpoint" form, 'taylor' its "heun" form.  Seed: `seed` (int in [0, 2**64)), or one
    draw from `generator`, or from torch's default CPU generator.  A callable `correcting_xt_fn` is applied after each
    update, i.e. after the noise."""
    check_solver(self, order)
    t_0 = 1. / self.noise_schedule.total_N if t_end is None else t_end
    t_T = self.noise_schedule.T if t_start is None else t_start
    assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
    seed = resolve_seed(seed, generator)
    check_state(self, x)
    plan = self._sample_plan(x, steps, t_0, t_T, order, skip_type, 'multistep', lower_order_final, denoise_to_zero,
                             solver_type, sde=True)
    DV._require_gpu(x)
    intermediates = []
    prev, grp = self._noise_seed, self._group
    self._noise_seed, self._group = seed, None
    try:
        with torch.no_grad():
            x = self._run_plan(plan, x, 'multistep', self.correcting_xt_fn, return_intermediate, intermediates)
    finally:
        self._noise_seed, self._group = prev, grp
    return (x, intermediates) if return_intermediate else x


def sample_sde_requests(self, xs, seeds=None, generator=None, steps=20, t_start=None, t_end=None, order=2,
                        skip_type='time_uniform', lower_order_final=True, denoise_to_zero=False, solver_type='dpmsolver',
                        return_intermediate=False):
    """(extension) `sample_sde` for several independent requests in flight together, each with its own seed: the list
    `[sample_sde(x, seed=s, ...) for x, s in zip(xs, seeds)]`, bit for bit.  `seeds`: one int in [0, 2**64) per request; None:
    one draw per request, in request order, from `generator` or from torch's default CPU generator (the call then equals
    len(xs) consecutive `sample_sde` calls).  The requests advance stage by stage -- the network once per request, then ONE
    fused kernel for all of them, every request's noise keyed by its own seed (dpm_stage_launch_multi).  A `correcting_xt_fn`
    written in Python, `return_intermediate`, a single request and requests of different shapes run one after the other."""
    xs = list(xs)
    check_solver(self, order)
    t_0 = 1. / self.noise_schedule.total_N if t_end is None else t_end
    t_T = self.noise_schedule.T if t_start is None else t_start
    assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
    if seeds is not None and generator is not None:
        raise ValueError("sample_sde_requests: pass either `seeds` or `generator`, not both")
    if seeds is not None:
        seeds = list(seeds)
        if len(seeds) != len(xs):
            raise ValueError("sample_sde_requests: %d seeds for %d requests" % (len(seeds), len(xs)))
        seeds = [resolve_seed(s, None) for s in seeds]
    else:
        seeds = [resolve_seed(None, generator) for _ in xs]
    for x in xs:
        check_state(self, x)
    kw = dict(steps=steps, t_start=t_start, t_end=t_end, order=order, skip_type=skip_type, lower_order_final=lower_order_final,
              denoise_to_zero=denoise_to_zero, solver_type=solver_type, return_intermediate=return_intermediate)
    together = (len(xs) > 1 and not return_intermediate and self.correcting_xt_fn is None
                and all(torch.is_tensor(x) and x.shape == xs[0].shape and x.dtype == xs[0].dtype and x.device == xs[0].device
                        for x in xs) and xs[0].dim() > 0 and xs[0].numel() > 0)
    if not together:
        return [self.sample_sde(x, seed=s, **kw) for x, s in zip(xs, seeds)]
    plan = self._sample_plan(xs[0], steps, t_0, t_T, order, skip_type, 'multistep', lower_order_final, denoise_to_zero,
                             solver_type, sde=True)
    DV._require_gpu(xs[0])
    prev = self._noise_seed, self._group, self._group_seeds
    self._noise_seed, self._group, self._group_seeds = None, xs, seeds
    try:
        with torch.no_grad():      # _run_plan picks the group up and returns the list of results
            return self._run_plan(plan, xs[0], 'multistep', None, False, [])
    finally:
        self._noise_seed, self._group, self._group_seeds = prev
