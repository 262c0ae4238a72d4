"""A strict model of the slab pool's copy stream -- TEST INFRASTRUCTURE, installed on top of table_double.install_table_double
or of a per-flavour double that builds on it (table_blend_double, table_thresh_double, table_rescale_double, ...).

tests/table_double.py copies synchronously and makes `_event_wait` a no-op: a pool that refilled a pinned ring slot too early
would still pass on it.  This model keeps the data path (a copy is performed at once, so every result keeps its bits) and adds
the OTHER extreme of the device's timing: the device is arbitrarily slow.  A copy has happened only once the host has waited on
an event recorded at or after it -- one stream, in order.  Until then the copy is *pending*, and the bytes of its pinned source
range must stay what they were when it was issued:

  _pinned_bytes    a plain CPU tensor, as in table_double; the model remembers it: the k-th buffer of a pool is ring slot k
  _copy_to_device  copies at once; records (sequence number, address and length of the source, a snapshot of its bytes) as
                   pending; returns a fake event that carries the sequence number
  _event_wait(ev)  marks every pending copy with a sequence number at or below ev's as passed; None passes nothing

The rule is checked at every _copy_to_device, at every _event_wait before it marks anything, around every DPM_TABLE_FILL and
DPM_TABLE_LAUNCH call of the multi-launch double underneath, and at the end of every SlabPool.step().  A violation raises
`Torn` with the tick, the ring slot (found from the address) and the first differing byte offset within the slot's pinned
buffer.  The stage and buffers arrays of a slot are never a copy's source, so they are free to change.

The model also keeps a log for the tests: `copies` -- (tick, sequence number, slot, offset within the slot, bytes) -- and
`waits` -- (tick, sequence number of the event waited on, or None)."""
import ctypes as C

import numpy as np
import torch

from dpm_solver_amd import _lib as L
from dpm_solver_amd import slab


class Torn(AssertionError):
    """a pending copy's pinned source changed before the host had waited for the copy"""

    def __init__(self, where, tick, issued, slot, offset, seq):
        self.where, self.tick, self.issued, self.slot, self.offset, self.seq = where, tick, issued, slot, offset, seq
        super().__init__("tick %d (%s): ring slot %s was rewritten at byte offset %d while copy #%d of tick %d, which reads "
                         "that byte, had not been waited for" % (tick, where, slot, offset, seq, issued))


class Event:
    """what _copy_to_device returns under the model: the copy's sequence number (the device never gets there by itself)"""

    def __init__(self, seq):
        self.seq = seq

    def query(self):
        return False


class _Pending:
    __slots__ = ("seq", "tick", "addr", "n", "snap")


def _bytes_at(addr, n):
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(addr))


class StagingModel:
    def __init__(self):
        self.pins = []          # every pinned buffer, in order of allocation (kept alive: addresses stay unique)
        self.pending = []
        self.seq = 0
        self.tick = -1          # the tick a step() is running (SlabPool._tick at its entry)
        self.copies, self.waits = [], []
        self.checks = 0

    # ---- the three hooks
    def pinned_bytes(self, n):
        t = torch.zeros(int(n), dtype=torch.uint8)
        self.pins.append(t)
        return t

    def copy_to_device(self, dst, src):
        self.check("_copy_to_device")
        assert src.dtype is torch.uint8 and src.is_contiguous()
        dst.copy_(src)
        p = _Pending()
        self.seq += 1
        p.seq, p.tick, p.addr, p.n = self.seq, self.tick, int(src.data_ptr()), int(src.numel())
        p.snap = _bytes_at(p.addr, p.n).copy()
        self.pending.append(p)
        slot, off = self.slot_of(p.addr)
        self.copies.append((self.tick, p.seq, slot, off, p.n))
        return Event(p.seq)

    def event_wait(self, ev):
        self.check("_event_wait")
        self.waits.append((self.tick, None if ev is None else ev.seq))
        if ev is not None:
            self.pending = [p for p in self.pending if p.seq > ev.seq]

    # ---- the rule
    def slot_of(self, addr):
        """(ring slot, byte offset within its pinned buffer) of a host address; (None, 0) for memory the model did not hand out"""
        for k, t in enumerate(self.pins):
            base = int(t.data_ptr())
            if base <= addr < base + t.numel():
                return k % slab._RING, addr - base
        return None, 0

    def check(self, where):
        self.checks += 1
        for p in self.pending:
            now = _bytes_at(p.addr, p.n)
            if not np.array_equal(now, p.snap):
                first = int(np.flatnonzero(now != p.snap)[0])
                slot, off = self.slot_of(p.addr)
                raise Torn(where, self.tick, p.tick, slot, off + first, p.seq)


def install_staging_double(monkeypatch, S):
    """on top of an installed table double (S: dpm_solver_amd.solver, which forwards to _device); returns the model"""
    m = StagingModel()
    under = S._stage_launch_multi_raw

    def launch_multi(st, bufs, n_req, stream):
        mode = int(bufs[0].opts.contents.table_mode) & (L.TABLE_FILL | L.TABLE_LAUNCH)
        what = {L.TABLE_FILL: "DPM_TABLE_FILL", L.TABLE_LAUNCH: "DPM_TABLE_LAUNCH"}.get(mode)
        if what:
            m.check("before " + what)
        rc = under(st, bufs, n_req, stream)
        if what:
            m.check("after " + what)
        return rc

    step = slab.SlabPool.step

    def checked_step(pool):
        m.tick = pool._tick
        out = step(pool)
        m.check("end of step()")
        return out

    monkeypatch.setattr(S, "_stage_launch_multi_raw", launch_multi)
    monkeypatch.setattr(S, "_pinned_bytes", m.pinned_bytes)
    monkeypatch.setattr(S, "_copy_to_device", m.copy_to_device)
    monkeypatch.setattr(S, "_event_wait", m.event_wait)
    monkeypatch.setattr(slab.SlabPool, "step", checked_step)
    return m
