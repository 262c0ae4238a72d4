"""model_wrapper -- host mirror of the reference function (dpm_solver_pytorch.py:170-334).

Same signature and semantics.  The returned object is callable like the reference's `model_fn(x,
t_continuous) -> noise`, but it also exposes the *raw* network outputs so that DPM_Solver can fuse the
parameterisation conversion (x_start / v / score -> noise, ref :288-298), the classifier-free-guidance
blend (ref :326-330) and the classifier-guidance term (ref :315-321) into the prologue of the stage
kernel instead of running them as separate elementwise passes.  The network itself (and the autograd
call through the classifier) stays an opaque PyTorch-ROCm call on the current stream.
"""
import copy
import math
import numbers

import torch

from .remedies import REMEDIES


class WrappedModel:
    # guidance rescale (Lin et al. 2023, section 3.4; diffusers' `guidance_rescale`): phi in [0, 1], set through
    # dpm_solver_amd.cfg_rescale -- model_wrapper's signature is the reference's.  0 = off: every bit as without it.
    guidance_rescale = 0.0
    # adaptive projected guidance (Sadat et al. 2024; diffusers' APG guider): (eta, norm threshold, momentum), set through
    # dpm_solver_amd.cfg_apg.  None = off: every bit as without it.
    guidance_apg = None
    # CFG-Zero* (Fan et al. 2025; diffusers' ClassifierFreeZeroStarGuidance): set through dpm_solver_amd.cfg_zero_star.
    # False = off: every bit as without it.
    guidance_zero_star = False
    # guidance over two conditions (InstructPix2Pix's image and text scales, composable conditions): (condition2, s1, s2), set
    # through dpm_solver_amd.cfg_pair.  None = off: every bit as without it.
    guidance_pair = None
    # Perp-Neg (Armandpour et al. 2023; ComfyUI's PerpNeg), set through dpm_solver_amd.cfg_perp_neg: guidance_pair is then
    # (negative_condition, guidance scale, negative scale) and the three outputs meet in the per-sample projection
    # (DPM_F_CFG2_PERP), not in cfg_pair's linear blend.  False = off: every bit as without it.
    guidance_perp = False
    _c_in3 = None                            # (condition2, the three conditions concatenated)

    def __init__(self, model, noise_schedule, model_type, model_kwargs, guidance_type, condition,
                 unconditional_condition, guidance_scale, classifier_fn, classifier_kwargs):
        self.model = model
        self.noise_schedule = noise_schedule
        self.model_type = model_type
        self.model_kwargs = model_kwargs
        self.guidance_type = guidance_type
        self.condition = condition
        self.unconditional_condition = unconditional_condition
        self.guidance_scale = guidance_scale
        self.classifier_fn = classifier_fn
        self.classifier_kwargs = classifier_kwargs
        self._c_in = None

    # ---- what the fused kernel must do for this wrapper -------------------------------------
    @property
    def effective_guidance(self):
        if self.guidance_type == "classifier":
            return "classifier"
        if self.pair is not None:
            return "classifier-free-2"           # (also at guidance_scale == 1: the second condition still guides)
        if self.guidance_type == "classifier-free" and not (
                self.guidance_scale == 1. or self.unconditional_condition is None):
            return "classifier-free"
        return "uncond"

    @property
    def pair(self):
        """(condition2, s1, s2) of the guidance over two conditions this wrapper asks the stage kernels for (include/dpm_hip.h,
        DPM_GUIDE_CFG2: eps = (n_u + s1 * (n_c - n_u)) + s2 * (n_c2 - n_u)); None = none"""
        if self.guidance_pair is None or self.guidance_type != "classifier-free" or self.unconditional_condition is None:
            return None
        return self.guidance_pair

    @property
    def perp(self):
        """does this wrapper ask the stage kernels for the Perp-Neg projection of its three outputs (include/dpm_hip.h,
        DPM_F_CFG2_PERP)?  `pair` is then (negative condition, s, w)"""
        return bool(self.guidance_perp) and self.pair is not None

    @property
    def rescale_phi(self):
        """phi of the guidance rescale this wrapper asks the stage kernels for; 0.0 = none (phi 0, or no classifier-free blend)"""
        phi = float(self.guidance_rescale)
        return phi if phi != 0.0 and self.effective_guidance == "classifier-free" else 0.0

    @property
    def apg(self):
        """(eta, norm threshold, momentum) of the adaptive projected guidance this wrapper asks the stage kernels for; None =
        none (never set, or no classifier-free blend)"""
        return self.guidance_apg if self.guidance_apg is not None and self.effective_guidance == "classifier-free" else None

    @property
    def zero_star(self):
        """does this wrapper ask the stage kernels for the CFG-Zero* projection?  False: never set, or no classifier-free blend"""
        return bool(self.guidance_zero_star) and self.effective_guidance == "classifier-free"

    def apg_x0(self, x, t_continuous, average=None):
        """The guided DATA prediction under adaptive projected guidance, in torch (include/dpm_hip.h, DPM_F_CFG_APG, in the
        tensors' own precision -- half outputs are widened to fp32 first, as the stage kernel widens them --, the three
        per-sample sums in float64).  `average`: the running average of the guidance direction, an fp32 tensor of x's shape
        updated in place (momentum != 0); None: a first step, the average starts at zero."""
        from .utils import expand_dims
        eta, r, beta = self.apg
        e0, e1, _ = self.raw_outputs(x, t_continuous)
        dims = x.dim()
        wide = torch.float64 if torch.float64 in (x.dtype, e0.dtype) else torch.float32
        e0, e1, xw = e0.to(wide), e1.to(wide), x.to(wide)
        alpha_t, sigma_t = self.noise_schedule.device_alpha_sigma(t_continuous)
        al, sg = expand_dims(alpha_t, dims).to(wide), expand_dims(sigma_t, dims).to(wide)
        mt = self.model_type

        def x0_of(out):                                           # noise_pred_fn (ref :288-298), then ref :439
            if mt == "x_start":
                eps = (xw - al * out) / sg
            elif mt == "v":
                eps = al * out + sg * xw
            elif mt == "score":
                eps = -sg * out
            else:
                eps = out
            return (xw - sg * eps) / al
        c = x0_of(e0)
        d = c - x0_of(e1)
        if beta != 0.0:
            if average is not None:
                d = average.copy_(d + beta * average.to(wide)).to(wide)
            # (no average: a first step -- d + beta * 0)
        axes = list(range(1, dims))
        d64, c64 = d.double(), c.double()
        s_dd = (d64 * d64).sum(dim=axes, keepdim=True)
        s_dc = (d64 * c64).sum(dim=axes, keepdim=True)
        s_cc = (c64 * c64).sum(dim=axes, keepdim=True)
        sc64 = torch.ones_like(s_dd)
        if r > 0.0:
            t = float(torch.tensor(r, dtype=torch.float32)) / s_dd.sqrt()
            sc64 = torch.where(t < 1.0, t, sc64)
        sc, q = sc64.to(wide), (sc64 * s_dc / s_cc).to(wide)
        dn, par = sc * d, q * c
        upd = (dn - par) + eta * par
        s1 = float(torch.tensor(float(self.guidance_scale), dtype=torch.float32) - 1.0)   # (s - 1.f) as the kernel forms it
        return c + s1 * upd

    def get_model_input_time(self, t_continuous):
        """ref :271-280"""
        if self.noise_schedule.schedule == 'discrete':
            return (t_continuous - 1. / self.noise_schedule.total_N) * 1000.
        return t_continuous

    def _cond_grad(self, x, t_input):
        """grad_x log p_t(cond | x_t) through the (opaque) classifier, ref :300-307"""
        with torch.enable_grad():
            x_in = x.detach().requires_grad_(True)
            log_prob = self.classifier_fn(x_in, t_input, self.condition, **self.classifier_kwargs)
            return torch.autograd.grad(log_prob.sum(), x_in)[0]

    def raw_outputs(self, x, t_continuous, t_input=None, t_input2=None, x_in2=None):
        """Run the network(s) exactly as the reference does and return (e0, e1, g):
        e0 raw output (conditional half under CFG), e1 raw unconditional output or None, g classifier
        gradient or None.  No conversion or blending is applied here -- the stage kernel does that."""
        if t_input is None:
            t_input = self.get_model_input_time(t_continuous)
        kw = self.model_kwargs
        if self.guidance_type == "uncond":
            return self.model(x, t_input, **kw), None, None
        if self.guidance_type == "classifier":
            assert self.classifier_fn is not None
            g = self._cond_grad(x, t_input)
            return self.model(x, t_input, **kw), None, g
        if self.guidance_type == "classifier-free":
            if self.pair is not None:
                # guidance over two conditions: ONE call on three copies of x, conditions ordered (uncond, condition,
                # condition2); returns (e0, e1, e2) -- e2 travels where the classifier gradient does (dpm_buffers.g)
                c3 = self._c_in3
                if c3 is None or c3[0] is not self.pair[0]:   # the conditioning does not change between steps: concatenate once
                    c3 = self._c_in3 = (self.pair[0], torch.cat([self.unconditional_condition, self.condition, self.pair[0]]))
                # t_input2: the tripled time the solver's loops keep per stage (DPM_Solver._time_views), like the doubled one below
                t_in = t_input2 if t_input2 is not None else torch.cat([t_input] * 3)
                e1, e0, e2 = self.model(torch.cat([x] * 3), t_in, c3[1], **kw).chunk(3)
                return e0, e1, e2
            if self.guidance_scale == 1. or self.unconditional_condition is None:
                return self.model(x, t_input, self.condition, **kw), None, None
            # x_in2: the stage kernel that produced x already wrote it into both halves of one [2B,...] buffer
            x_in = x_in2 if x_in2 is not None else torch.cat([x] * 2)
            t_in = t_input2 if t_input2 is not None else torch.cat([t_input] * 2)
            if self._c_in is None:  # the conditioning does not change between steps: concatenate once
                self._c_in = torch.cat([self.unconditional_condition, self.condition])
            out = self.model(x_in, t_in, self._c_in, **kw)
            e1, e0 = out.chunk(2)
            return e0, e1, None
        raise AssertionError(self.guidance_type)

    # ---- reference-compatible call: noise prediction ------------------------------------------
    def __call__(self, x, t_continuous):
        """The reference's model_fn(x, t_continuous) -> noise (ref :282-330) for callers OTHER than DPM_Solver (which fuses
        these conversions into its stage kernels and never comes here): the raw network call(s), then the reference's own
        tensor expressions in torch on x's device -- per-sample times (`t_continuous` of shape (B,) with distinct entries)
        included, no host synchronisation (the schedule is evaluated on the device, NoiseScheduleVP.device_alpha_sigma).
        Under adaptive projected guidance (cfg_apg) the result is the noise prediction equivalent to the guided data
        prediction, (x - alpha * x0) / sigma; a direct call has no history: it is a FIRST step, with a running average of
        zero, whatever the momentum.  Under CFG-Zero* (cfg_zero_star) the unconditional RAW output is scaled by its
        per-sample least-squares fit to the conditional one before the blend (include/dpm_hip.h, DPM_F_CFG_ZSTAR)."""
        from .utils import expand_dims
        from ._device import _require_gpu
        _require_gpu(x)
        if self.apg is not None:
            x0 = self.apg_x0(x, t_continuous)
            alpha_t, sigma_t = self.noise_schedule.device_alpha_sigma(t_continuous)
            al, sg = expand_dims(alpha_t, x.dim()).to(x0.dtype), expand_dims(sigma_t, x.dim()).to(x0.dtype)
            return (x.to(x0.dtype) - al * x0) / sg
        e0, e1, g = self.raw_outputs(x, t_continuous)
        mt = self.model_type
        dims = x.dim()

        def to_noise(out):                                        # noise_pred_fn, ref :288-298
            if mt == "noise":
                return out
            alpha_t, sigma_t = self.noise_schedule.device_alpha_sigma(t_continuous)
            if mt == "x_start":
                return (x - expand_dims(alpha_t, dims) * out) / expand_dims(sigma_t, dims)
            if mt == "v":
                return expand_dims(alpha_t, dims) * out + expand_dims(sigma_t, dims) * x
            return -expand_dims(sigma_t, dims) * out              # "score"
        eff = self.effective_guidance
        if eff == "classifier-free-2" and self.perp:
            # Perp-Neg, the torch statement of the contract (include/dpm_hip.h, DPM_F_CFG2_PERP): projection and blend on the RAW
            # outputs, the conversion afterwards; half outputs are widened to fp32 first, as the stage kernel widens them, and
            # nothing after that is rounded to half; the two per-sample sums in float64, their quotient rounded once to the
            # outputs' dtype, 0 where the positive direction vanishes
            o_c, o_u, o_n = e0, e1, g
            if o_c.dtype in (torch.float16, torch.bfloat16):
                o_c, o_u, o_n = o_c.float(), o_u.float(), o_n.float()
                x = x.float()
            _, s, w = self.pair
            if o_c.dtype is torch.float32:
                s, w = (float(torch.tensor(float(v), dtype=torch.float32)) for v in (s, w))
            axes = list(range(1, dims))
            d0, d2 = o_c - o_u, o_n - o_u
            p64, q64 = d0.double(), d2.double()
            s_nd = (q64 * p64).sum(dim=axes, keepdim=True)
            s_dd = (p64 * p64).sum(dim=axes, keepdim=True)
            a = torch.where(s_dd > 0, s_nd / s_dd, torch.zeros_like(s_dd)).to(o_c.dtype)
            perp = d2 - a * d0
            return to_noise(o_u + s * (d0 - w * perp))
        if eff == "classifier-free-2":
            # guidance over two conditions, the torch statement of the contract (include/dpm_hip.h, DPM_GUIDE_CFG2): half
            # outputs are widened to fp32 first, as the stage kernel widens them, the conversions per output, then the five
            # operations with both scales as fp32 values; nothing is rounded to half
            e2 = g
            if e0.dtype in (torch.float16, torch.bfloat16):
                e0, e1, e2 = e0.float(), e1.float(), e2.float()
                x = x.float()
            _, s1, s2 = self.pair
            if e0.dtype is torch.float32:
                s1, s2 = (float(torch.tensor(float(s), dtype=torch.float32)) for s in (s1, s2))
            n0, n1, n2 = to_noise(e0), to_noise(e1), to_noise(e2)
            return (n1 + s1 * (n0 - n1)) + s2 * (n2 - n1)
        if eff == "classifier":                                   # ref :315-321
            _, sigma_t = self.noise_schedule.device_alpha_sigma(t_continuous)
            return to_noise(e0) - self.guidance_scale * expand_dims(sigma_t, dims) * g
        if eff == "classifier-free" and self.rescale_phi != 0.0:
            # guidance rescale: blend and statistics on the RAW outputs (the paper, diffusers), the conversion afterwards; the
            # per-sample standard deviations in float64, their ratio rounded once to the outputs' dtype (include/dpm_hip.h)
            phi = self.rescale_phi
            half = e0.dtype in (torch.float16, torch.bfloat16)
            if half and mt != "noise":                   # such outputs meet the fp32 schedule first without rescale (ref :290-298):
                e0, e1 = e0.float(), e1.float()          # their blend is fp32 here too
            g = e1 + self.guidance_scale * (e0 - e1)     # a noise network: in its own dtype, like the blend without rescale (ref :330)
            if half:
                g = g.float()                            # nothing after the blend is rounded to half (as in the stage kernel)
            axes = list(range(1, dims))
            f = (e0.double().std(dim=axes, keepdim=True) / g.double().std(dim=axes, keepdim=True)).to(g.dtype)
            return to_noise(phi * (g * f) + (1. - phi) * g)
        if eff == "classifier-free" and self.zero_star:
            # CFG-Zero*: projection and blend on the RAW outputs, the conversion afterwards (include/dpm_hip.h, DPM_F_CFG_ZSTAR):
            # half outputs are widened to fp32 first, as the stage kernel widens them, and nothing after that is rounded to
            # half; the two per-sample sums in float64, their quotient rounded once to the outputs' dtype
            if e0.dtype in (torch.float16, torch.bfloat16):
                e0, e1 = e0.float(), e1.float()
            axes = list(range(1, dims))
            c64, u64 = e0.double(), e1.double()
            s_cu = (c64 * u64).sum(dim=axes, keepdim=True)
            s_uu = (u64 * u64).sum(dim=axes, keepdim=True)
            a = (s_cu / (s_uu + 1e-8)).to(e0.dtype)
            u = a * e1
            s = float(torch.tensor(float(self.guidance_scale), dtype=torch.float32)) if e0.dtype is torch.float32 else self.guidance_scale
            return to_noise(u + s * (e0 - u))
        if eff == "classifier-free":                              # ref :326-330
            nu, nc = to_noise(e1), to_noise(e0)
            return nu + self.guidance_scale * (nc - nu)
        return to_noise(e0)


def _classifier_free(helper, model_fn):
    """what every remedy helper asks first: `model_fn` is the result of model_wrapper(..., guidance_type='classifier-free')"""
    if not isinstance(model_fn, WrappedModel) or model_fn.guidance_type != "classifier-free":
        raise ValueError("%s: takes the result of model_wrapper(..., guidance_type='classifier-free'), got %s"
                         % (helper, getattr(model_fn, "guidance_type", None) or type(model_fn).__name__))


def _alone(helper, model_fn):
    """... and last, unless called with its identity setting: no other row's attribute is set; returns the copy to set its own on"""
    for r in REMEDIES:
        if r.name != helper and getattr(model_fn, r.raw):
            raise NotImplementedError("%s on top of %s: the two remedies are not built together" % (helper, r.name))
    if getattr(model_fn, "guidance_perp", False) and getattr(model_fn, "guidance_pair", None) is not None:
        raise NotImplementedError("%s on top of cfg_perp_neg: the Perp-Neg stage kernel has no remedy (a follow-up)" % helper)
    if getattr(model_fn, "guidance_pair", None) is not None:
        raise NotImplementedError("%s on top of cfg_pair: the two-condition stage kernel has no remedy (a follow-up)" % helper)
    return copy.copy(model_fn)


def apg_params(eta, norm_threshold, momentum):
    """cfg_apg's arguments, checked (its ranges and texts: a slab pool's submit(apg=...) goes through here too), as floats"""
    for name, v in (("eta", eta), ("norm_threshold", norm_threshold), ("momentum", momentum)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != v:
            raise ValueError("cfg_apg: %s must be a real number, got %r" % (name, v))
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError("cfg_apg: eta must be in [0, 1], got %r" % (eta,))
    if not (0.0 <= float(norm_threshold) < float("inf")):
        raise ValueError("cfg_apg: norm_threshold must be a finite number >= 0 (0 = off), got %r" % (norm_threshold,))
    if not -1.0 < float(momentum) < 1.0:
        raise ValueError("cfg_apg: momentum must be in (-1, 1), got %r" % (momentum,))
    return float(eta), float(norm_threshold), float(momentum)


def cfg_rescale(model_fn, phi):
    """(extension) A copy of the classifier-free wrapper `model_fn` with guidance rescale phi (Lin et al. 2023, "Common
    Diffusion Noise Schedules and Sample Steps Are Flawed", section 3.4; the `guidance_rescale` of diffusers pipelines): the
    guided output is rescaled so that its per-sample standard deviation matches the conditional output's, and blended with the
    un-rescaled one -- phi * rescaled + (1 - phi) * guided.  What v-prediction / zero-terminal-SNR checkpoints need at the
    usual guidance scales.  DPM_Solver runs it inside the stage kernel (DPM_F_CFG_RESCALE); phi = 0 changes nothing."""
    _classifier_free("cfg_rescale", model_fn)
    if isinstance(phi, bool) or not isinstance(phi, numbers.Real) or not (0.0 <= float(phi) <= 1.0):
        raise ValueError("cfg_rescale: phi must be a real number in [0, 1], got %r" % (phi,))
    out = _alone("cfg_rescale", model_fn) if phi else copy.copy(model_fn)
    out.guidance_rescale = float(phi)
    return out


def cfg_apg(model_fn, eta=0.0, norm_threshold=0.0, momentum=0.0):
    """(extension) A copy of the classifier-free wrapper `model_fn` with adaptive projected guidance (Sadat et al. 2024,
    "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models"; the APG guider of diffusers): the
    guidance direction -- conditional minus unconditional data prediction -- is capped at the per-sample norm `norm_threshold`
    (0 = no cap), split into its components parallel and orthogonal to the conditional prediction, the parallel one scaled by
    `eta` in [0, 1], and with `momentum` in (-1, 1) replaced by its running average over the network evaluations of a run
    (a = d + momentum * a; the paper uses negative values).  DPM_Solver runs it inside the stage kernel (DPM_F_CFG_APG) of the
    data-prediction samplers.  cfg_apg(fn, 1.0, 0.0, 0.0) is classifier-free guidance itself and changes nothing."""
    _classifier_free("cfg_apg", model_fn)
    params = apg_params(eta, norm_threshold, momentum)
    if params == (1.0, 0.0, 0.0):
        params = None                                        # classifier-free guidance itself
    out = _alone("cfg_apg", model_fn) if params else copy.copy(model_fn)
    out.guidance_apg = params
    return out


def cfg_zero_star(model_fn):
    """(extension) A copy of the classifier-free wrapper `model_fn` with the CFG-Zero* projection (Fan et al. 2025, "CFG-Zero*:
    Improved Classifier-Free Guidance for Flow Matching Models"; diffusers' `ClassifierFreeZeroStarGuidance`, ComfyUI's
    `CFGZeroStar`, which applies it to noise-prediction checkpoints as well): before the blend the unconditional output is
    scaled by its per-sample least-squares fit to the conditional one, a = <o_c, o_u> / ||o_u||^2, and the guided output is
    a * o_u + s * (o_c - a * o_u).  It carries no parameter.  DPM_Solver runs it inside the stage kernel (DPM_F_CFG_ZSTAR), for
    both algorithm types; at guidance scale 1 or without an unconditional condition it changes nothing.  The paper's
    "zero-init" -- a zero velocity in the first steps -- is NOT part of it: that is defined for flow-matching velocities and
    has no counterpart for a VP noise prediction."""
    _classifier_free("cfg_zero_star", model_fn)
    out = _alone("cfg_zero_star", model_fn)
    out.guidance_zero_star = True
    return out


def cfg_pair(model_fn, condition2, scale2, nested=False):
    """(extension) A copy of the classifier-free wrapper `model_fn` with guidance over TWO conditions: the network is evaluated
    on three copies of the input -- unconditional, `condition` (the wrapper's), `condition2` -- and the three outputs are blended
    inside the stage kernel (DPM_GUIDE_CFG2, stage_pair_kernel), in fp32.  With s = the wrapper's guidance_scale:
      nested=False (composable conditions):  e_u + s (e_c - e_u) + scale2 (e_c2 - e_u)
      nested=True (InstructPix2Pix):         e_u + scale2 (e_c2 - e_u) + s (e_c - e_c2) -- `condition` carries BOTH conditions
                                             (image and text), `condition2` the inner one alone (the image); scale2 is the image
                                             scale, s the text scale
    Both are (e_u + s1 (e_c - e_u)) + s2 (e_c2 - e_u) with s1 = s and s2 = scale2 (composable) or scale2 - s (nested, formed in
    double and rounded once).  s2 == 0 is classifier-free guidance itself: a plain copy, no third branch.  Not together with
    cfg_rescale / cfg_apg / cfg_zero_star, in either order.
    The three conditions are IMMUTABLE for the life of the returned wrapper: they are concatenated once, at the first
    evaluation, the solver's caches of plans, launch records and graphs know `condition2` by identity, and a captured graph
    replays the concatenation it was recorded with -- an edit in place would go unnoticed.  For another condition call
    cfg_pair again and give the result to a new DPM_Solver."""
    _classifier_free("cfg_pair", model_fn)
    if model_fn.unconditional_condition is None:
        raise ValueError("cfg_pair: takes a classifier-free wrapper with an unconditional_condition")
    if not torch.is_tensor(condition2):
        raise ValueError("cfg_pair: condition2 must be a tensor like the wrapper's condition, got %s" % type(condition2).__name__)
    if torch.is_tensor(model_fn.condition) and condition2.shape != model_fn.condition.shape:
        raise ValueError("cfg_pair: condition2 has shape %s, the wrapper's condition %s"
                         % (tuple(condition2.shape), tuple(model_fn.condition.shape)))
    if isinstance(scale2, bool) or not isinstance(scale2, numbers.Real) or not math.isfinite(float(scale2)):
        raise ValueError("cfg_pair: scale2 must be a finite real number, got %r" % (scale2,))
    if not isinstance(nested, bool):
        raise ValueError("cfg_pair: nested must be a bool, got %r" % (nested,))
    s = model_fn.guidance_scale
    if isinstance(s, bool) or not isinstance(s, numbers.Real) or not math.isfinite(float(s)):
        raise ValueError("cfg_pair: the wrapper's guidance_scale must be a finite real number, got %r" % (s,))
    for r in REMEDIES:
        if getattr(model_fn, r.raw):
            raise NotImplementedError("cfg_pair on top of %s: the two-condition stage kernel has no remedy (a follow-up)" % r.name)
    if model_fn.guidance_perp and model_fn.guidance_pair is not None:
        raise NotImplementedError("cfg_pair on top of cfg_perp_neg: the Perp-Neg stage kernel takes one negative condition and no "
                                  "second blend (a follow-up)")
    s1, s2 = float(s), (float(scale2) - float(s) if nested else float(scale2))
    out = copy.copy(model_fn)
    out._c_in3 = None                                         # (the copy concatenates its own conditions)
    out.guidance_pair = None if s2 == 0.0 else (condition2, s1, s2)
    return out


def cfg_perp_neg(model_fn, negative_condition, neg_scale=1.0):
    """(extension) A copy of the classifier-free wrapper `model_fn` with Perp-Neg guidance (Armandpour et al. 2023, "Re-imagine
    the Negative Prompt Algorithm"; ComfyUI's `PerpNeg` / `PerpNegGuider`).  The wrapper's `condition` is the positive prompt,
    its `unconditional_condition` the EMPTY prompt, `negative_condition` the negative prompt.  The network is evaluated on three
    copies of the input -- empty, positive, negative -- and, per image, the negative direction loses its component along the
    positive one before it is subtracted, so that a negative prompt that overlaps the positive one no longer erases the subject.
    With s = the wrapper's guidance_scale, d_pos = o_pos - o_empty and d_neg = o_neg - o_empty on the raw outputs:
      a = <d_neg, d_pos> / ||d_pos||^2 over the image;   guided = o_empty + s * (d_pos - neg_scale * (d_neg - a * d_pos))
    DPM_Solver runs it inside the stage kernel (DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 stage, stage_perp_kernel), in fp32, for both
    algorithm types.  neg_scale == 0 is classifier-free guidance itself: a plain copy, no third branch.  Not together with
    cfg_rescale / cfg_apg / cfg_zero_star / cfg_pair, in either order.  The three conditions are IMMUTABLE for the life of the
    returned wrapper, as under cfg_pair."""
    _classifier_free("cfg_perp_neg", model_fn)
    if model_fn.unconditional_condition is None:
        raise ValueError("cfg_perp_neg: takes a classifier-free wrapper with an unconditional_condition (the empty prompt)")
    if not torch.is_tensor(negative_condition):
        raise ValueError("cfg_perp_neg: negative_condition must be a tensor like the wrapper's condition, got %s"
                         % type(negative_condition).__name__)
    if torch.is_tensor(model_fn.condition) and negative_condition.shape != model_fn.condition.shape:
        raise ValueError("cfg_perp_neg: negative_condition has shape %s, the wrapper's condition %s"
                         % (tuple(negative_condition.shape), tuple(model_fn.condition.shape)))
    if isinstance(neg_scale, bool) or not isinstance(neg_scale, numbers.Real) or not math.isfinite(float(neg_scale)):
        raise ValueError("cfg_perp_neg: neg_scale must be a finite real number, got %r" % (neg_scale,))
    s = model_fn.guidance_scale
    if isinstance(s, bool) or not isinstance(s, numbers.Real) or not math.isfinite(float(s)):
        raise ValueError("cfg_perp_neg: the wrapper's guidance_scale must be a finite real number, got %r" % (s,))
    for r in REMEDIES:
        if getattr(model_fn, r.raw):
            raise NotImplementedError("cfg_perp_neg on top of %s: the Perp-Neg stage kernel has no remedy (a follow-up)" % r.name)
    if model_fn.guidance_pair is not None:
        raise NotImplementedError("cfg_perp_neg on top of %s: the Perp-Neg stage kernel takes one negative condition and no "
                                  "second blend (a follow-up)" % ("cfg_perp_neg" if model_fn.guidance_perp else "cfg_pair"))
    out = copy.copy(model_fn)
    out._c_in3 = None                                         # (the copy concatenates its own conditions)
    w = float(neg_scale)
    out.guidance_pair = None if w == 0.0 else (negative_condition, float(s), w)
    out.guidance_perp = w != 0.0
    return out


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond",
                  condition=None, unconditional_condition=None, guidance_scale=1., classifier_fn=None,
                  classifier_kwargs={}):
    """Create a wrapper function for the noise prediction model (signature of ref :170-181).

    model_type: "noise" | "x_start" | "v" | "score";  guidance_type: "uncond" | "classifier" |
    "classifier-free".  Returns `model_fn(x, t_continuous) -> noise`.
    """
    assert model_type in ["noise", "x_start", "v", "score"]
    assert guidance_type in ["uncond", "classifier", "classifier-free"]
    return WrappedModel(model, noise_schedule, model_type, model_kwargs, guidance_type, condition,
                        unconditional_condition, guidance_scale, classifier_fn, classifier_kwargs)
