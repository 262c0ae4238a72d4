"""guarded launches of a Perp-Neg stage (DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 record) -- TEST INFRASTRUCTURE, never imported by
the product.  The operands are pair_guarded.PairLaunch's: e0 (positive), e1 (unconditional) and g (negative), each in a guarded
arena of its own.  Here: the case builder with the outputs given as VALUES (the correlated draw, the anchors), and the run of the
numpy double (tests/perp_double.py), which asserts on the CPU that a does not depend on the summation order before it computes."""
import kernel_double as KD
import pair_guarded as PG
import perp_double as PP
import guarded as G


class _Pristine:
    def __init__(self, pristine):
        self.pristine = pristine


def bits(values, dt):
    t = values.to(dt)
    return t.view(G._INT[t.element_size()])


def values(b, dt):
    return b.view(dt).float()


def make_case(st, n, batch, sd, ed, outputs=None, like=None, **kw):
    """a PairLaunch of `st`; outputs: None -- three independent normal outputs (the arenas' own draw); else
    f(e0, e1, g) -> (e0, e1, g) on fp32 tensors of the drawn values, stored in the network's dtype"""
    mk = lambda lk: PG.PairLaunch("perp", st, n, sd, ed, batch=batch, like=lk, **kw)
    case = mk(like)
    if outputs is None or like is not None:
        return case
    pr = dict(case.pristine)
    e0, e1, g = outputs(*(values(pr[k], ed) for k in ("e0", "e1", "g")))
    pr["e0"], pr["e1"], pr["g"] = bits(e0, ed), bits(e1, ed), bits(g, ed)
    return mk(_Pristine(pr))


def run_double(case, check=True):
    """run the numpy double on (CPU) `case` -- its inputs asserted decidable first --, check that it stayed inside its payloads,
    return the case"""
    assert PP.launch_raw_double(KD._Ref(case.st), KD._Ref(case.b), None, check=check) == 0
    case.verify()
    return case
