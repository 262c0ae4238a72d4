"""UniPC sampling: `DPM_Solver.sample_unipc` (extension; Zhao et al. 2023, diffusers' `UniPCMultistepScheduler`), data-prediction
form, order 1 or 2, variants 'bh1' / 'bh2'.

One network evaluation per step, like the multistep solvers: step i predicts x_i^p, evaluates m_i = model(x_i^p, t_i) and
corrects x_i^p to x_i with it; m_i is also what step i+1 starts from.  Predictor and corrector of a step share their
first-order part, so the corrected state is the predicted one plus a combination of model-value differences, and it is
consumed by the next predictor only: stage i of the plan (dpm_plan_create with DPM_ALGO_UNIPC; include/dpm_hip.h,
DPM_FORM_UNIPC) runs the corrector of step i AND the predictor of step i+1 in one kernel -- it reads x_i^p, the network
output and one or two cached model values and writes x_{i+1}^p and m_i, the streams of a third-order multistep stage.  The
corrected states leave the kernel only for `return_intermediate` (DPM_F_STORE_XC).

With the corrector off the predictor of 'bh2', order 2, IS DPM-Solver++ 2M: `corrector=False` runs sample()'s multistep plan.
With it on, the step orders follow UniPC's rule o_i = min(order, i, steps + 1 - i) at every step count (`lower_order_final`),
where sample() lowers the final orders below 10 steps only.
"""
import torch

from . import _device as DV
from . import _lib as L


def check_solver(self, order, variant):
    """sample_unipc's errors about the solver, the order and the variant (shared with sample_unipc_requests)"""
    if self.algorithm_type != "dpmsolver++":
        raise NotImplementedError("sample_unipc: algorithm_type='dpmsolver' (the noise-prediction UniPC) is not built; "
                                  "use algorithm_type='dpmsolver++'")
    self._check_remedies("sample_unipc -- the UniPC stage kernels have no {noun} (a follow-up)")
    self._check_pair("sample_unipc -- the UniPC stage kernels blend two network outputs, not three (a follow-up)")
    if self._thresholding:
        raise NotImplementedError("sample_unipc: correcting_x0_fn='dynamic_thresholding' -- the thresholding kernel has no "
                                  "UniPC form")
    if self._user_x0 is not None:
        raise NotImplementedError("sample_unipc: a callable correcting_x0_fn (the stage would be split around it; the UniPC "
                                  "stages have no such split)")
    if self.correcting_xt_fn is not None:
        raise NotImplementedError("sample_unipc: correcting_xt_fn -- the corrector works on the predicted state the network "
                                  "saw, which must reach the next stage untouched")
    if order not in (1, 2):
        raise ValueError("sample_unipc: 'order' must be 1 or 2, got {} (order 3 needs a third cached model value in "
                         "dpm_buffers: a follow-up)".format(order))
    if variant not in L.UNIPC_VARIANT:
        raise ValueError("sample_unipc: 'variant' must be either 'bh1' or 'bh2', got {}".format(variant))


def check_state(self, x):
    if self._sdtype(x) is torch.float64:
        raise NotImplementedError("sample_unipc: double-precision states (there is no double UniPC kernel)")


def _times(self, t_start, t_end):
    t_0 = 1. / self.noise_schedule.total_N if t_end is None else t_end
    t_T = self.noise_schedule.T if t_start is None else t_start
    assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
    return t_0, t_T


def sample_unipc(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', variant='bh2',
                 corrector=True, lower_order_final=True, denoise_to_zero=False, return_intermediate=False):
    """Sample by UniPC (multistep, order 1 or 2, data prediction) from x_T at `t_start` to `t_end` with `steps` network
    evaluations.  `steps`, `t_start`, `t_end`, `skip_type`, `denoise_to_zero` mean what they mean for
    `sample(method='multistep')`; `variant` is UniPC's B(h): 'bh1' (h) or 'bh2' (expm1(h), diffusers' default).
    `corrector=False` is the predictor alone -- for 'bh2' that is sample()'s multistep DPM-Solver++ plan (solver_type
    'dpmsolver'), bit for bit.  `return_intermediate` returns (x, [x_1, ..., x_{steps-1}, final state(s)]): the CORRECTED
    states, then the last step's state (and the denoised one with `denoise_to_zero`)."""
    check_solver(self, order, variant)
    t_0, t_T = _times(self, t_start, t_end)
    check_state(self, x)
    if not corrector:
        if variant != 'bh2':
            raise NotImplementedError("sample_unipc: corrector=False with variant='bh1' (the predictor alone is built for "
                                      "'bh2', where it is DPM-Solver++ 2M)")
        return self.sample(x, steps=steps, t_start=t_start, t_end=t_end, order=order, skip_type=skip_type, method='multistep',
                           lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero, solver_type='dpmsolver',
                           return_intermediate=return_intermediate)
    plan = self._sample_plan(x, steps, t_0, t_T, order, skip_type, 'multistep', lower_order_final, denoise_to_zero,
                             'dpmsolver', unipc=variant)
    DV._require_gpu(x)
    if self.auto_capture and self._group is None and not torch.cuda.is_current_stream_capturing():
        hit = self._auto_captured(x, dict(unipc=True, method='multistep', steps=steps, t_start=t_start, t_end=t_end, order=order,
                                          skip_type=skip_type, variant=variant, lower_order_final=lower_order_final,
                                          denoise_to_zero=denoise_to_zero), return_intermediate)
        if hit is not None:
            return hit
    intermediates = []
    with torch.no_grad():
        x = self._run_plan(plan, x, 'multistep', None, return_intermediate, intermediates)
    return (x, intermediates) if return_intermediate else x


def sample_unipc_requests(self, xs, steps=20, t_start=None, t_end=None, order=2, skip_type='time_uniform', variant='bh2',
                          corrector=True, lower_order_final=True, denoise_to_zero=False, return_intermediate=False):
    """(extension) `sample_unipc` for several independent requests in flight together: the list
    `[sample_unipc(x, ...) for x in xs]`, bit for bit.  The requests advance stage by stage -- the network once per request,
    then ONE fused kernel for all of them (dpm_stage_launch_multi).  `return_intermediate`, a single request and requests of
    different shapes run one after the other."""
    xs = list(xs)
    check_solver(self, order, variant)
    t_0, t_T = _times(self, t_start, t_end)
    for x in xs:
        check_state(self, x)
    kw = dict(steps=steps, t_start=t_start, t_end=t_end, order=order, skip_type=skip_type, variant=variant, corrector=corrector,
              lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero, return_intermediate=return_intermediate)
    together = (len(xs) > 1 and not return_intermediate and corrector
                and all(torch.is_tensor(x) and x.shape == xs[0].shape and x.dtype == xs[0].dtype and x.device == xs[0].device
                        for x in xs) and xs[0].dim() > 0 and xs[0].numel() > 0)
    if not corrector:
        if variant != 'bh2':
            return [self.sample_unipc(x, **kw) for x in xs]       # (its NotImplementedError)
        return self.sample_requests(xs, steps=steps, t_start=t_start, t_end=t_end, order=order, skip_type=skip_type,
                                    method='multistep', lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero,
                                    solver_type='dpmsolver', return_intermediate=return_intermediate)
    if not together:
        return [self.sample_unipc(x, **kw) for x in xs]
    plan = self._sample_plan(xs[0], steps, t_0, t_T, order, skip_type, 'multistep', lower_order_final, denoise_to_zero,
                             'dpmsolver', unipc=variant)
    DV._require_gpu(xs[0])
    prev = self._group
    self._group = xs
    try:
        with torch.no_grad():      # _run_plan picks the group up and returns the list of results
            return self._run_plan(plan, xs[0], 'multistep', None, False, [])
    finally:
        self._group = prev
