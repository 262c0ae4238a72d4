"""SDE-DPM-Solver++ sampling: `DPM_Solver.sample_sde` (extension; "DPM++ 2M SDE", diffusers' `sde-dpmsolver++`).

The plan is `sample(method='multistep')`'s plan -- same stages, forms, times, buffer roles and history slots -- with the
stochastic update's scalars (dpm_plan_create with DPM_ALGO_SDE_DPMSOLVERPP): every first- / second-order stage adds
sigma_t * sqrt(1 - e^{-2h}) * z, z generated INSIDE the stage kernel by a counter-based generator (Philox4x32-10 keyed by the
seed, counter = element index and stage index: include/dpm_hip.h, "noise contract").  No noise tensor is written or read and
no launch is added: an SDE stage moves the bytes of the ODE stage.  The seed travels per call in dpm_launch_opts, so the
prebuilt launch records (_FastRun) and the plan cache never hold it, and the call bypasses auto_capture (a replayed graph
would bake one seed in).
"""
import torch

from . import _device as DV

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


def sample_sde(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', lower_order_final=True,
               denoise_to_zero=False, solver_type='dpmsolver', seed=None, generator=None, return_intermediate=False):
    """Sample by SDE-DPM-Solver++ (multistep, order 1 or 2) from x_T at `t_start` to `t_end`.  `steps`, `t_start`, `t_end`,
    `skip_type`, `lower_order_final`, `denoise_to_zero` mean what they mean for `sample(method='multistep')`;
    solver_type 'dpmsolver' is diffusers' "midpoint" form, 'taylor' its "heun" form.  Seed: `seed` (int in [0, 2**64)), or one
    draw from `generator`, or from torch's default CPU generator.  A callable `correcting_xt_fn` is applied after each
    update, i.e. after the noise."""
    if self.algorithm_type != "dpmsolver++":
        raise NotImplementedError("sample_sde: algorithm_type='dpmsolver' (the noise-prediction SDE variant) is not built; "
                                  "use algorithm_type='dpmsolver++'")
    if self._thresholding:
        raise NotImplementedError("sample_sde: correcting_x0_fn='dynamic_thresholding' -- the thresholding kernel has no noise "
                                  "epilogue")
    if self._user_x0 is not None:
        raise NotImplementedError("sample_sde: a callable correcting_x0_fn (the stage would be split around it; the SDE "
                                  "stages have no such split)")
    if order not in (1, 2):
        raise ValueError("sample_sde: 'order' must be 1 or 2 (no third-order SDE update is defined), got {}".format(order))
    t_0 = 1. / self.noise_schedule.total_N if t_end is None else t_end
    t_T = self.noise_schedule.T if t_start is None else t_start
    assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
    seed = resolve_seed(seed, generator)
    if self._sdtype(x) is torch.float64:
        raise NotImplementedError("sample_sde: double-precision states (there is no double noise kernel)")
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
