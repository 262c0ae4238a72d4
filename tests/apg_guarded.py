"""the fp32 running-average arena of a DPM_F_CFG_APG launch next to a guarded.GuardedLaunch -- TEST INFRASTRUCTURE, never
imported by the product.  The average travels in dpm_buffers.workspace, is read AND written in place, and is fp32 whatever the
state's dtype: an arena of its own (guard | n fp32 values | guard, at the launch's offset), not GuardedLaunch's zero-filled
thresholding workspace."""
import torch

import guarded as G


def attach(case, bits=None):
    """give `case` (a GuardedLaunch) a running-average arena holding the int32 bit patterns `bits` -- None: the arena's fill
    pattern, a poison no launch without a momentum may read or write -- and point the record's workspace at it"""
    case.avg = G.Arena(torch.float32, case.n, case.device, case.offset, bits=bits)
    case.avg_pristine = bits
    case.b.workspace = case.avg.ptr
    return case


def random_bits(n, seed):
    v = torch.randn(n, generator=torch.Generator().manual_seed(7919 * seed + 5))
    return v.view(torch.int32)


def on(case, device):
    """the same case, pristine, on `device`, its average arena included"""
    return attach(case.on(device), case.avg_pristine)


def verify(dev, want=None, rc=0):
    """GuardedLaunch.verify plus the average: guards intact, the payload the double's bits (want given and a momentum), else
    untouched"""
    dev.verify(want, rc=rc)
    dev.avg.verify("average", None if (want is None or rc != 0 or dev.st.thr_max == 0.0) else want.avg.payload_bits())
