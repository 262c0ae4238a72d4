"""The classifier-free remedies as one family, without a GPU: every case of tests/remedy_cases.py answers what the fixture
recorded before the host plumbing became one table (tests/golden/remedy_refusals.json: exception type and FULL text, or the
bound stage records byte for byte), the cache key tells every kind and setting apart, and the table's flags are the three."""
import itertools

import pytest

import dpm_solver_amd as D
import remedy_cases as RC
from dpm_solver_amd import _lib as L
from dpm_solver_amd import remedies as R

FIXTURE = RC.load_fixture()["cases"]


def test_fixture_and_cases_name_the_same_ids():
    assert sorted(FIXTURE) == sorted(RC.CASES)


@pytest.mark.parametrize("cid", list(RC.CASES))
def test_case_answers_what_the_parent_answered(monkeypatch, cid):
    assert list(RC.run_case(RC.CASES[cid], monkeypatch)) == FIXTURE[cid]


def _solvers():
    """name -> a function that builds a solver: every kind on every wrapper, and no kind at all"""
    out = {"off": lambda: D.DPM_Solver(*RC.wrapper()), "no_wrapper": lambda: D.DPM_Solver(lambda x, t: x, RC.make_schedule("sd"))}
    for kind in RC.KINDS:
        for w, wkw in RC.WRAPPERS.items():
            out["%s/%s" % (kind, w)] = lambda kind=kind, wkw=wkw: D.DPM_Solver(*RC._wrapped((kind,), **wkw))
    out["rescale_0.5/on"] = lambda: D.DPM_Solver(D.cfg_rescale(RC.wrapper()[0], 0.5), RC.make_schedule("sd"))
    return out


def test_remedy_key_is_equal_for_equal_settings_and_distinct_otherwise():
    make = _solvers()
    keys = {name: f()._remedy_key() for name, f in make.items()}
    for name, f in make.items():
        assert f()._remedy_key() == keys[name] and hash(f()._remedy_key()) == hash(keys[name])
    off = keys["off"]
    assert keys["no_wrapper"] == off and all(keys["%s/%s" % (k, w)] == off for k in RC.KINDS for w in ("scale1", "no_uncond"))
    distinct = ["off", "rescale_0.5/on"] + ["%s/on" % k for k in RC.KINDS]
    for a, b in itertools.combinations(distinct, 2):
        assert keys[a] != keys[b], (a, b)
    # ... and several kinds at once (set behind the helpers' backs) differ from each of them alone
    both = D.DPM_Solver(*RC._wrapped(("rescale", "zstar")))._remedy_key()
    assert both not in (keys["rescale/on"], keys["zstar/on"], off)


def test_active_rows_come_in_table_order_with_their_settings():
    assert D.DPM_Solver(*RC.wrapper())._remedies() == []
    got = D.DPM_Solver(*RC._wrapped(("zstar", "apg_mom", "rescale")))._remedies()
    assert [(r.name, v) for r, v in got] == [("cfg_rescale", 0.7), ("cfg_apg", (0.5, 0.0, -0.5)), ("cfg_zero_star", True)]


def test_table_flags_are_the_three():
    assert [r.name for r in R.REMEDIES] == ["cfg_rescale", "cfg_apg", "cfg_zero_star"]
    assert [r.flag for r in R.REMEDIES] == [L.F_CFG_RESCALE, L.F_CFG_APG, L.F_CFG_ZSTAR]
    assert R.F_CFG_REMEDIES == L.F_CFG_RESCALE | L.F_CFG_APG | L.F_CFG_ZSTAR
