"""a guarded.GuardedLaunch for a stage under guidance over two conditions (DPM_GUIDE_CFG2) -- TEST INFRASTRUCTURE, never imported
by the product.  Such a launch reads THREE network outputs: e0 (the condition), e1 (unconditional) and g (the second condition),
all of the eps dtype and all dense.  GuardedLaunch knows e1 under classifier-free guidance and g under classifier guidance only;
this subclass owns both next to e0, each in a guarded arena of its own at the launch's offset, and verifies them as inputs."""
import torch

import guarded as G
import kernel_double as KD
import pair_double as PD
from dpm_solver_amd import _lib as L


class PairLaunch(G.GuardedLaunch):
    EXTRA = ("e1", "g")

    def __init__(self, family, st, n, sd, ed, device="cpu", like=None, without=(), **kw):
        """without: operands of EXTRA the record leaves NULL (the error cases)"""
        assert st.guidance == L.GUIDE["classifier-free-2"] and not kw.get("stride")
        super().__init__(family, st, n, sd, ed, device=device, like=like, **kw)
        self.without = tuple(without)
        gen = torch.Generator().manual_seed(1000003 * self.kw["seed"] + 7 * self.req + 3)
        for k in self.EXTRA:
            if like is not None:
                bits = like.pristine[k]
            else:
                v = torch.randn(self.n, generator=gen).to(ed)
                bits = v.view(G._INT[v.element_size()])
            self.pristine[k] = bits
            self.arenas[k] = G.Arena(ed, self.n, device, self.offset, bits=bits)
        self.b = self.buffers()
        for k in self.without:
            setattr(self.b, k, None)

    def on(self, device):
        return PairLaunch(self.family, self.st, self.n, self.sd, self.ed, device=device, like=self, without=self.without, **self.kw)

    def share(self, dst, src):
        """operand `dst` of the record points at the arena of `src` (g == e1, e0 == e1 == g: the anchors)"""
        setattr(self.b, dst, self.arenas[src].ptr)
        return self


def run_double(case):
    """run the numpy double on (CPU) `case`, check that it stayed inside its payloads, return the case"""
    assert PD.launch_raw_double(KD._Ref(case.st), KD._Ref(case.b), None) == 0
    case.verify()
    return case
