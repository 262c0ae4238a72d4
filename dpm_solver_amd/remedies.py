"""The classifier-free "remedies" -- guidance rescale, adaptive projected guidance, CFG-Zero* -- as ONE table (DESIGN section
4): a row holds what differs between kinds; the functions are everything the host does with a kind besides its math (wrapper.py):
read its setting, refuse what it is not built with, bind it into a stage record, key the caches.  They take the DPM_Solver as
`self`; solver.py binds the first four as `_remedies`, `_remedy_setting`, `_remedy_key` and `_check_remedies`."""
from collections import namedtuple

import torch

from . import _device as DV
from . import _lib as L


def _bind_rescale(st, phi):
    """a classifier-free stage record carries DPM_F_CFG_RESCALE and phi in `cg_scale` -- a field the planner writes and no
    classifier-free kernel reads"""
    if st.guidance == L.GUIDE["classifier-free"]:
        _, cg, fl = DV._cfg_fields(st.cfg_scale, phi, st.sigma_e, st.flags)
        st.cg_scale, st.flags = float(cg), int(fl)


def _bind_apg(st, apg):
    """a classifier-free stage record carries DPM_F_CFG_APG, eta in `cg_scale`, the norm threshold in `thr_ratio` and the
    momentum in `thr_max` -- fields nothing else reads under the flag.  (The running average travels in dpm_buffers.workspace,
    in a DPM_TABLE_APG call in dpm_buffers.thr_hint: the caller binds it.)"""
    if st.guidance == L.GUIDE["classifier-free"]:
        cg, ratio, mx, fl = DV._apg_fields(apg[0], apg[1], apg[2], (st.cg_scale, st.thr_ratio, st.thr_max), st.flags)
        st.cg_scale, st.thr_ratio, st.thr_max, st.flags = float(cg), float(ratio), float(mx), int(fl)


def _bind_zstar(st, on):
    """a classifier-free stage record carries DPM_F_CFG_ZSTAR and nothing else -- the flag reads cfg_scale alone"""
    if st.guidance == L.GUIDE["classifier-free"]:
        st.flags |= L.F_CFG_ZSTAR


# name: the helper;  title, label: what messages call the kind;  flag: its stage flag;  attr: the WrappedModel property that
# reads its setting -- falsy = off (0.0, None, False: never set, or no classifier-free blend);  raw: the attribute the helper
# sets;  bind(stage record, setting);  needs_x0: defined on the data prediction alone;  noun: what a kernel family without the
# kind "has no";  stages: the adjective of its stages;  blend / double / together / slab: its clause for a MaskBlend corrector, a
# double state, a second kind, a slab pool;  switch: the request_pool(slots=...) switch that admits it
Remedy = namedtuple("Remedy", "name title label flag attr raw bind needs_x0 noun stages blend double together slab switch")
# name: the keyword;  excludes: (another switch, why);  needs: why a classifier-free wrapper;  kernel: what has no other epilogue
Switch = namedtuple("Switch", "name excludes needs kernel")


def _row(name, title, *a, **kw):
    return Remedy(name, title, "%s (%s)" % (title, name), *a, **kw)


REMEDIES = (
    _row("cfg_rescale", "guidance rescale", L.F_CFG_RESCALE, "rescale_phi", "guidance_rescale", _bind_rescale,
         needs_x0=False, noun="rescale", stages="rescale",
         blend="the rescale kernel has no mask-blend epilogue (a follow-up)", double="there is no double rescale kernel",
         together=None,                          # (the first row: a later kind refuses it)
         slab="rescale stages take the table in a pool built with request_pool(slots=..., rescale=True) only",
         switch=Switch("rescale", (("sde", "the SDE stage kernels have no rescale"),
                                   ("thresholding", "the thresholding kernels have no rescale"),
                                   ("inpaint", "the rescale kernel has no mask-blend epilogue")),
                       "guidance rescale rescales the guided output", "the rescale kernel")),
    _row("cfg_apg", "adaptive projected guidance", L.F_CFG_APG, "apg", "guidance_apg", _bind_apg,
         needs_x0=True, noun="projected guidance", stages="projected-guidance",
         blend="its kernel has no mask-blend epilogue (a follow-up)", double="there is no double kernel",
         together="the two remedies are not built together",
         slab="projected-guidance stages take the table in a pool built with request_pool(slots=..., apg=True) only; a "
              "RequestPool (no slots) takes a cfg_apg solver as it is",
         switch=Switch("apg", (("rescale", "the APG kernel has no guidance rescale"),
                               ("sde", "the APG kernel has no noise epilogue"),
                               ("thresholding", "the APG kernel has no thresholding"),
                               ("inpaint", "the APG kernel has no mask-blend epilogue")),
                       "adaptive projected guidance projects the guidance direction", "the APG kernel")),
    _row("cfg_zero_star", "CFG-Zero*", L.F_CFG_ZSTAR, "zero_star", "guidance_zero_star", _bind_zstar,
         needs_x0=False, noun="CFG-Zero* projection", stages="CFG-Zero*",
         blend="its kernel has no mask-blend epilogue (a follow-up)", double="there is no double kernel",
         together="the remedies are not built together",
         slab="CFG-Zero* stages have no table row kind yet (a follow-up); a RequestPool (no slots) takes a cfg_zero_star "
              "solver as it is",
         switch=Switch("zero_star", (("rescale", "the CFG-Zero* kernel has no guidance rescale"),
                                     ("apg", "the CFG-Zero* kernel has no projected guidance"),
                                     ("sde", "the CFG-Zero* kernel has no noise epilogue"),
                                     ("thresholding", "the CFG-Zero* kernel has no thresholding"),
                                     ("inpaint", "the CFG-Zero* kernel has no mask-blend epilogue")),
                       "CFG-Zero* projects the unconditional output onto the conditional one", "the CFG-Zero* kernel")),
)
F_CFG_REMEDIES = sum(r.flag for r in REMEDIES)     # (distinct bits: their OR) what the prologue half of a split stage keeps


def active(self):
    """[(row, setting), ...] of the active kinds in table order: none or one, unless attributes were set behind the helpers' backs"""
    w = self._wrapped
    rows = [] if w is None else [(r, getattr(w, r.attr)) for r in REMEDIES]
    return [(r, v) for r, v in rows if v]


def setting(self, name):
    """the setting of the kind `name`, None = off: for what one kind alone has (APG's running average, a slab row's defaults)"""
    return dict((r.name, v) for r, v in active(self)).get(name)


def key(self):
    """what the caches of launch records and graphs key on: changes with any kind or setting"""
    return tuple((r.name, v) for r, v in active(self))


def thresholded(r):
    """the refusal of a thresholded stage under the kind `r`"""
    return NotImplementedError("%s: correcting_x0_fn='dynamic_thresholding' -- the thresholding kernels have no %s (a "
                               "follow-up)" % (r.label, r.noun))


def check(self, what=None, sd=None, blend=False, only=None):
    """The combinations the active kinds are not built with, kind by kind in table order.  `what` names a
    sampler or a mode without remedy kernels ({noun} / {stages} in it: the row's); else the solver-wide rules, then the run's
    corrector (`blend`) and state dtype (`sd`).  Called once where a run starts and by _run_stage, whose state dtype the first
    evaluation may have promoted; a thresholded stage is refused where it is bound (_prep_stage).  `only`: that kind alone."""
    rows = active(self)
    for i, (r, _) in enumerate(rows):
        if only is not None and r.name != only:
            continue
        if what is not None:
            raise NotImplementedError("%s: %s" % (r.label, what.format(noun=r.noun, stages=r.stages)))
        if i:
            raise NotImplementedError("%s: together with %s -- %s" % (r.label, rows[0][0].label, r.together))
        if r.needs_x0 and self.algorithm_type != "dpmsolver++":
            raise NotImplementedError("%s: algorithm_type='dpmsolver' -- it is defined on the data prediction "
                                      "(algorithm_type='dpmsolver++')" % r.label)
        if r.needs_x0 and self._thresholding:                 # (every evaluating stage of such a solver is thresholded)
            raise thresholded(r)
        if blend:
            raise NotImplementedError("%s: a MaskBlend corrector -- %s" % (r.label, r.blend))
        if sd is torch.float64:
            raise NotImplementedError("%s: double-precision states (%s)" % (r.label, r.double))


def check_switches(self, slots, on):
    """request_pool's switches that admit a kind (`on`: every switch by name): a slab pool's, a classifier-free wrapper's, and
    not with the switches -- or on the solvers -- its kernel has no epilogue for"""
    for r in REMEDIES:
        sw = r.switch
        if sw is None or not on[sw.name]:
            continue
        if slots is None:
            raise ValueError("request_pool: %s=True belongs to a slab pool (slots=...); a RequestPool takes a %s solver as it is"
                             % (sw.name, r.name))
        for other, why in sw.excludes:
            if on[other]:
                raise NotImplementedError("request_pool: %s=True with %s=True -- %s (a follow-up)" % (sw.name, other, why))
        if self._wrapped is None or self._wrapped.effective_guidance != "classifier-free":
            raise ValueError("request_pool: %s=True needs a classifier-free wrapper (an unconditional condition and a guidance "
                             "scale other than 1): %s" % (sw.name, sw.needs))
        if r.needs_x0 and self.algorithm_type != "dpmsolver++":
            raise NotImplementedError("request_pool: %s=True with algorithm_type='dpmsolver' -- %s is defined on the data "
                                      "prediction (algorithm_type='dpmsolver++')" % (sw.name, r.title))
        clash = ["correcting_x0_fn='dynamic_thresholding'"] if r.needs_x0 and self._thresholding else []
        clash += [q.name for q, _ in active(self) if q.switch is not None and q.switch.name in dict(sw.excludes)]
        if clash:                        # (a solver that IS what an excluded switch admits)
            raise NotImplementedError("request_pool: %s=True on a solver with %s -- %s has none of those epilogues (a follow-up)"
                                      % (sw.name, clash[0], sw.kernel))


def check_slab(self, on):
    """a slab pool takes an active kind only through its switch (`on`: the pool's switches by name)"""
    for r, _ in active(self):
        if r.switch is None or not on.get(r.switch.name):
            raise NotImplementedError("%s: the slab pool (request_pool(slots=...)) -- %s" % (r.label, r.slab))
