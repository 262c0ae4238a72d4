"""The classifier-free remedies (cfg_rescale, cfg_apg, cfg_zero_star) as cases: what every public entry point answers under
each kind -- ("ok",) or (exception type name, full message) -- and the stage records the binder builds, as hex.  TEST
INFRASTRUCTURE: public API and the CPU doubles only, so the same file runs on any commit; tests/golden/remedy_refusals.json is
its output on the commit named in that file's first line, and tests/test_remedies_host.py compares the two.

    PYTHONPATH=.:tests/golden python tests/remedy_cases.py <commit>        rewrites the fixture from the checked-out tree

The CPU doubles are kernel_double's and, per kind, rescale_double / apg_double / zstar_double; the SDE and UniPC situations take
sde_double / unipc_double (under an active kind they refuse before any launch; where the kind is off they run).  capture() is
asked what it refuses: the graph itself (GraphedSample) is stubbed.
"""
import json
import os
import sys

import pytest
import torch

import dpm_solver_amd as D
import dpm_solver_amd.solver as S
import apg_double as AD
import rescale_double as RD
import sde_double as SD
import unipc_double as UD
import zstar_double as ZD
from engine_cases import make_schedule

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "remedy_refusals.json")

# the kinds: (helper call, raw attribute to set behind the helpers' backs, the CPU double of its stages)
KINDS = {
    "rescale": (lambda fn: D.cfg_rescale(fn, 0.7), ("guidance_rescale", 0.7), RD.install_rescale_double),
    "apg_cap": (lambda fn: D.cfg_apg(fn, 0.5, 10.0, 0.0), ("guidance_apg", (0.5, 10.0, 0.0)), AD.install_apg_double),
    "apg_mom": (lambda fn: D.cfg_apg(fn, 0.5, 0.0, -0.5), ("guidance_apg", (0.5, 0.0, -0.5)), AD.install_apg_double),
    "zstar": (D.cfg_zero_star, ("guidance_zero_star", True), ZD.install_zstar_double),
}
WRAPPERS = {"on": {}, "scale1": dict(scale=1.0), "no_uncond": dict(uncond=False)}   # the two last: every kind is off


def _net(x, t, c):
    return torch.tanh(x * 0.7) * (0.5 + 0.1 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]) + 0.05 * x + 0.2 * c.reshape(-1, 1, 1, 1)[:x.shape[0]]


def wrapper(model_type="noise", scale=3.0, uncond=True):
    ns = make_schedule("sd")
    c = torch.ones(2)
    return D.model_wrapper(_net, ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=scale, condition=c,
                           unconditional_condition=c * 0 if uncond else None), ns


def _x():
    return torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(0))


def _t(v):
    return torch.tensor([v])


def _blend(x):
    return D.MaskBlend(make_schedule("sd"), torch.ones(8, 8), x0=x, noise=x)


# ------------------------------------------------------------------------------------------------
# the situations: name -> (function of (mk, x), double to install or None for the kind's own); mk(**kw) builds the solver
# ------------------------------------------------------------------------------------------------
RUN = dict(steps=6, order=2)
SITUATIONS = {
    "sample": (lambda mk, x: mk().sample(x, **RUN), None),
    "sample_requests": (lambda mk, x: mk().sample_requests([x, x + 1], **RUN), None),
    "sample_adaptive": (lambda mk, x: mk().sample(x, method="adaptive", **RUN), None),
    "dpm_solver_adaptive": (lambda mk, x: mk().dpm_solver_adaptive(x, 2, 1.0, 1e-3), None),
    "sample_sde": (lambda mk, x: mk().sample_sde(x, steps=6, seed=1), SD.install_sde_double),
    "sample_sde_requests": (lambda mk, x: mk().sample_sde_requests([x, x], steps=6, seeds=[1, 2]), SD.install_sde_double),
    "sample_unipc": (lambda mk, x: mk().sample_unipc(x, steps=6), UD.install_unipc_double),
    "sample_unipc_requests": (lambda mk, x: mk().sample_unipc_requests([x, x], steps=6), UD.install_unipc_double),
    "slab": (lambda mk, x: mk().request_pool(slots=8), None),
    "slab_rescale": (lambda mk, x: mk().request_pool(slots=8, rescale=True), None),
    "slab_apg": (lambda mk, x: mk().request_pool(slots=8, apg=True), None),
    "slab_sde": (lambda mk, x: mk().request_pool(slots=8, sde=True), None),
    "slab_thresholding": (lambda mk, x: mk().request_pool(slots=8, thresholding=True), None),
    "slab_thresholding_solver": (lambda mk, x: mk(correcting_x0_fn="dynamic_thresholding").request_pool(slots=8, thresholding=True), None),
    "slab_inpaint": (lambda mk, x: mk().request_pool(slots=8, inpaint=True), None),
    "slab_rescale_apg": (lambda mk, x: mk().request_pool(slots=8, rescale=True, apg=True), None),
    "switch_rescale_without_slots": (lambda mk, x: mk().request_pool(rescale=True), None),
    "switch_apg_without_slots": (lambda mk, x: mk().request_pool(apg=True), None),
    "pool_submit": (lambda mk, x: mk().request_pool().submit(x, steps=6), None),
    "pool_submit_sde": (lambda mk, x: mk().request_pool().submit(x, steps=6, sde=True, seed=3), SD.install_sde_double),
    "pool_submit_unipc": (lambda mk, x: mk().request_pool().submit_unipc(x, steps=6), UD.install_unipc_double),
    "thresholding_sample": (lambda mk, x: mk(correcting_x0_fn="dynamic_thresholding").sample(x, **RUN), None),
    "thresholding_data_prediction": (lambda mk, x: mk(correcting_x0_fn="dynamic_thresholding").data_prediction_fn(x, _t(0.5)), None),
    "thresholding_noise_prediction": (lambda mk, x: mk(correcting_x0_fn="dynamic_thresholding").noise_prediction_fn(x, _t(0.5)), None),
    "thresholding_pool_submit": (lambda mk, x: mk(correcting_x0_fn="dynamic_thresholding").request_pool().submit(x, steps=6), None),
    "maskblend": (lambda mk, x: mk(correcting_xt_fn=_blend(x)).sample(x, **RUN), None),
    "double_sample": (lambda mk, x: mk().sample(x.double(), **RUN), None),
    "double_sample_requests": (lambda mk, x: mk().sample_requests([x.double(), x.double()], **RUN), None),
    "double_pool_submit": (lambda mk, x: mk().request_pool().submit(x.double(), steps=6), None),
    "double_data_prediction": (lambda mk, x: mk().data_prediction_fn(x.double(), _t(0.5)), None),
    "dpmsolver_sample": (lambda mk, x: mk(algorithm_type="dpmsolver").sample(x, **RUN), None),
    "dpmsolver_pool_submit": (lambda mk, x: mk(algorithm_type="dpmsolver").request_pool().submit(x, steps=6), None),
    "dpmsolver_first_update": (lambda mk, x: mk(algorithm_type="dpmsolver").dpm_solver_first_update(x, _t(0.8), _t(0.6)), None),
    "dpmsolver_model_fn": (lambda mk, x: mk(algorithm_type="dpmsolver").model_fn(x, _t(0.5)), None),
    "data_prediction": (lambda mk, x: mk().data_prediction_fn(x, _t(0.5)), None),
    "capture": (lambda mk, x: mk().capture(x, **RUN), None),
    "capture_thresholding": (lambda mk, x: mk(correcting_x0_fn="dynamic_thresholding").capture(x, **RUN), None),
}
# several kinds active at once (set behind the helpers' backs): which reason wins
TOGETHER = ("sample", "maskblend", "double_sample", "thresholding_sample", "dpmsolver_sample", "pool_submit", "sample_sde",
            "sample_adaptive", "data_prediction", "capture")
BASE = ("rescale", "apg_cap", "zstar")


def _slab(**switches):
    return D.DPM_Solver(*wrapper()).request_pool(slots=8, **switches)


# a slab pool's submit: the request's own remedy without the pool's switch, and apg= with each argument cfg_apg rejects
SLAB_SUBMIT = {
    "rescale_without_switch": lambda x: _slab().submit(x, steps=6, guidance_rescale=0.7),
    "rescale_in_an_apg_pool": lambda x: _slab(apg=True).submit(x, steps=6, guidance_rescale=0.7),
    "apg_without_switch": lambda x: _slab().submit(x, steps=6, apg=(0.5, 10.0, 0.0)),
    "apg_in_a_rescale_pool": lambda x: _slab(rescale=True).submit(x, steps=6, apg=(0.5, 10.0, 0.0)),
    "apg_on_an_uncond_wrapper": lambda x: D.DPM_Solver(*wrapper(scale=1.0)).request_pool(slots=8).submit(x, steps=6, apg=(0.5, 0.0, 0.0)),
}
BAD_APG = {"not_a_triple": (0.5, 10.0), "a_number": 0.5, "eta_low": (-0.1, 0.0, 0.0), "eta_high": (1.5, 0.0, 0.0),
           "eta_nan": (float("nan"), 0.0, 0.0), "eta_str": ("0.5", 0.0, 0.0), "eta_none": (None, 0.0, 0.0),
           "eta_bool": (True, 0.0, 0.0), "r_negative": (0.5, -1.0, 0.0), "r_inf": (0.5, float("inf"), 0.0),
           "r_nan": (0.5, float("nan"), 0.0), "r_complex": (0.5, 1j, 0.0), "momentum_1": (0.5, 0.0, 1.0),
           "momentum_minus_1": (0.5, 0.0, -1.0), "momentum_nan": (0.5, 0.0, float("nan")), "momentum_str": (0.5, 0.0, "x")}
for _name, _apg in BAD_APG.items():
    SLAB_SUBMIT["apg_%s" % _name] = lambda x, a=_apg: _slab(apg=True).submit(x, steps=6, apg=a)
    SLAB_SUBMIT["apg_%s_without_switch" % _name] = lambda x, a=_apg: _slab().submit(x, steps=6, apg=a)


def _helpers():
    """the helpers' own errors: a non-wrapper argument, every 'on top of' pair in both orders, the identities"""
    ns = make_schedule("sd")
    fn = lambda: wrapper()[0]
    bad = {"function": lambda: (lambda x, t: x), "uncond_wrapper": lambda: D.model_wrapper(lambda x, t: x, ns),
           "classifier_wrapper": lambda: D.model_wrapper(lambda x, t: x, ns, guidance_type="classifier",
                                                         classifier_fn=lambda *a: 0, condition=torch.ones(1))}
    out = {}
    for kind in BASE:
        for name, make in bad.items():
            out["%s_of_a_%s" % (kind, name)] = lambda kind=kind, make=make: KINDS[kind][0](make())
        for under in BASE:
            if under != kind:
                out["%s_on_top_of_%s" % (kind, under)] = lambda kind=kind, under=under: KINDS[kind][0](KINDS[under][0](fn()))
                out["%s_on_top_of_%s_scale1" % (kind, under)] = (
                    lambda kind=kind, under=under: KINDS[kind][0](KINDS[under][0](wrapper(scale=1.0)[0])))
    out["apg_mom_on_top_of_rescale"] = lambda: KINDS["apg_mom"][0](KINDS["rescale"][0](fn()))
    for under in BASE:                                       # the identities refuse nothing, in either order
        out["rescale_0_on_top_of_%s" % under] = lambda under=under: D.cfg_rescale(KINDS[under][0](fn()), 0.0)
        out["apg_identity_on_top_of_%s" % under] = lambda under=under: D.cfg_apg(KINDS[under][0](fn()), 1.0, 0.0, 0.0)
        out["%s_on_top_of_rescale_0" % under] = lambda under=under: KINDS[under][0](D.cfg_rescale(fn(), 0.0))
        out["%s_on_top_of_apg_identity" % under] = lambda under=under: KINDS[under][0](D.cfg_apg(fn(), 1.0, 0.0, 0.0))
    out["rescale_phi_out_of_range"] = lambda: D.cfg_rescale(fn(), 1.5)
    out["rescale_phi_bool"] = lambda: D.cfg_rescale(fn(), True)
    for name, apg in BAD_APG.items():
        if isinstance(apg, tuple) and len(apg) == 3:
            out["apg_%s" % name] = lambda apg=apg: D.cfg_apg(fn(), *apg)
            out["apg_%s_on_top_of_rescale" % name] = lambda apg=apg: D.cfg_apg(KINDS["rescale"][0](fn()), *apg)
    return out


HELPERS = _helpers()
MODEL_TYPES = ("noise", "x_start", "v")
ALGORITHMS = ("dpmsolver", "dpmsolver++")


def _cases():
    """id -> the case as data: ('run', kinds, wrapper, situation) | ('slab_submit', name) | ('helper', name) |
    ('records', kind, model type, algorithm type)"""
    out = {}
    for kind in KINDS:
        for w in WRAPPERS:
            for sit in SITUATIONS:
                out["%s/%s/%s" % (kind, w, sit)] = ("run", (kind,), w, sit)
    pairs = [(a, b) for a in BASE for b in BASE if a != b] + [("rescale", "apg_mom"), BASE, BASE[::-1]]
    for kinds in pairs:
        for sit in TOGETHER:
            out["%s/on/%s" % ("+".join(kinds), sit)] = ("run", tuple(kinds), "on", sit)
    for name in SLAB_SUBMIT:
        out["slab_submit/%s" % name] = ("slab_submit", name)
    for name in HELPERS:
        out["helper/%s" % name] = ("helper", name)
    for kind in KINDS:
        for mt in MODEL_TYPES:
            for algo in ALGORITHMS:
                if algo == "dpmsolver++" or not kind.startswith("apg"):     # (where the kind is allowed)
                    out["records/%s/%s/%s" % (kind, mt, algo)] = ("records", kind, mt, algo)
    return out


CASES = _cases()


def _wrapped(kinds, **wkw):
    """the wrapper under kinds[0]'s helper, the rest set behind the helpers' backs"""
    fn, ns = wrapper(**wkw)
    fn = KINDS[kinds[0]][0](fn)
    for k in kinds[1:]:
        setattr(fn, *KINDS[k][1])
    return fn, ns


def _records(kind, model_type, algorithm_type):
    """hex of every dpm_stage of a 6-step 2M plan after _prep_stage, guidance scale 3"""
    fn, ns = _wrapped((kind,), model_type=model_type)
    dpm = D.DPM_Solver(fn, ns, algorithm_type=algorithm_type)
    plan = dpm._get_plan(method="multistep", order=2, steps=6, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=ns.T, t_0=1.0 / ns.total_N)
    return [bytes(dpm._prep_stage(ps.copy())).hex() for ps in plan.stages]


def run_case(case, monkeypatch):
    """("ok",) | (exception type name, full message) | ("records", hex, ...)"""
    try:
        if case[0] == "records":
            return ("records",) + tuple(_records(*case[1:]))
        if case[0] == "helper":
            HELPERS[case[1]]()
            return ("ok",)
        if case[0] == "slab_submit":
            AD.install_apg_double(monkeypatch, S, D)
            SLAB_SUBMIT[case[1]](_x())
            return ("ok",)
        _, kinds, w, sit = case
        fn, install = SITUATIONS[sit]
        (install or KINDS[kinds[0]][2])(monkeypatch, S, D)
        monkeypatch.setattr(S, "GraphedSample", lambda *a, **kw: "captured")    # capture(): what it refuses, not the graph
        wrapped, ns = _wrapped(kinds, **WRAPPERS[w])
        fn(lambda **kw: D.DPM_Solver(wrapped, ns, **kw), _x())
        return ("ok",)
    except Exception as e:       # noqa: BLE001  (the case's answer: type and text)
        return (type(e).__name__, str(e))


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    got = {}
    for cid, case in CASES.items():
        with pytest.MonkeyPatch.context() as mp:
            got[cid] = list(run_case(case, mp))
    with open(FIXTURE, "w") as f:
        f.write('{"recorded_from": %s, "cases": {\n' % json.dumps(sys.argv[1]))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in got.items()))
        f.write("\n}}\n")
    print("%d cases -> %s" % (len(got), FIXTURE))
