"""The churn scenario of a slab pool that holds EVERY kind of request at once -- TEST INFRASTRUCTURE, shared by
tests/test_slab_mixed_host.py (numpy doubles) and tests/test_gpu_slab_mixed.py (MI355X).

request_pool(slots=12, sde=True, inpaint=True): 36 requests of four kinds -- plain multistep, UniPC, SDE, inpainting -- come in
over ten ticks, four per tick for nine ticks.  They cannot all fit: the FIFO of waiting requests is exercised, and a freed row
goes to the next request in line, whatever its kind.  The order of the kinds (ORDER) is chosen so that, by the pool's own
admission rule restated in `simulate`,

  * every ordered pair (kind that freed a row -> kind admitted into it), the four same-kind pairs included, occurs,
  * the lowest active row -- whose options are the call's own, seed included -- is held by each of the four kinds on some tick,
  * some tick has all four kinds active, and some request waits two ticks or more.

`simulate` is a restatement: the tests that run the scenario compare it, tick by tick, with the rows the real pool handed out.
"""
import torch

KINDS = ("plain", "unipc", "sde", "blend")
SLOTS, SHAPE = 12, (4, 16, 16)
PER_TICK = 4                                   # submissions per tick
# the kind of request j, P(lain) U(niPC) S(DE) I(npainting)
ORDER = "UISIUISISPUPPUSPPIUPPUPSISIISPSUUSIU"
_KIND = dict(zip("PUSI", KINDS))
SEEDS = (0, (1 << 63) + 5, 77, 0xFEEDFACE12345678, 1 << 32)


def specs(order=ORDER, per_tick=PER_TICK):
    """request j as a dict: tick of submission, kind, b in {1, 3}, the keyword arguments of its submit (steps 4..9; orders 1..3
    for plain and inpainting requests, 1..2 for UniPC -- both variants -- and SDE; denoise_to_zero on some), an SDE request's
    seed (0 and one beyond 2^63 among them), an inpainting request's MaskBlend mode and mask shape"""
    out = []
    for j, c in enumerate(order):
        kind, k = _KIND[c], order[:j].count(c)            # k: the request's number among those of its kind
        b = 1 + 2 * ((k + k // 2) % 2)
        kw = dict(steps=4 + (5 * j) % 6, denoise_to_zero=(k % 3 == 1))
        sp = dict(j=j, tick=j // per_tick, kind=kind, b=b, kw=kw)
        if kind == "unipc":
            kw.update(order=1 + k % 2, variant=("bh2", "bh1")[(k // 2) % 2])
        elif kind == "sde":
            kw.update(order=1 + (k // 2) % 2, seed=SEEDS[k % len(SEEDS)])
        else:
            kw.update(order=1 + k % 3, skip_type=("time_uniform", "logSNR")[k % 4 == 0])
        if kind == "blend":
            sp.update(mode=("x0", "intermediates")[k % 2], full_mask=bool((k // 2) % 2))
        out.append(sp)
    return out


def n_stages(sp):
    """ticks request `sp` stays in its rows: one stage per step, and the DENOISE stage of denoise_to_zero"""
    return sp["kw"]["steps"] + bool(sp["kw"]["denoise_to_zero"])


def simulate(sps, slots=SLOTS):
    """SlabPool's admission restated: per tick, submissions join the queue; the head of the queue is admitted while it fits,
    into the lowest free rows; every active request advances one stage and one at its last stage frees its rows.
    Returns (ticks, admitted): ticks[t] = {row: j} of the rows active on tick t, admitted[j] = the tick that admitted j."""
    free, wait, left, rows_of, ticks, admitted = list(range(slots)), [], {}, {}, [], {}
    t = 0
    while t <= max(sp["tick"] for sp in sps) or wait or rows_of:
        wait += [sp for sp in sps if sp["tick"] == t]
        while wait and wait[0]["b"] <= len(free):
            sp = wait.pop(0)
            rows_of[sp["j"]], free = free[:sp["b"]], free[sp["b"]:]
            left[sp["j"]], admitted[sp["j"]] = n_stages(sp), t
        ticks.append({r: j for j, rows in rows_of.items() for r in rows})
        for j in list(rows_of):
            left[j] -= 1
            if left[j] == 0:
                free = sorted(free + rows_of.pop(j))
        t += 1
    return ticks, admitted


def handovers(sps, ticks):
    """the set of (kind that held a row, kind that holds it next)"""
    out, last = set(), {}
    for occ in ticks:
        for r, j in occ.items():
            if r in last and last[r] != j:
                out.add((sps[last[r]]["kind"], sps[j]["kind"]))
            last[r] = j
    return out


def kinds_active(sps, occ):
    return {sps[j]["kind"] for j in occ.values()}


def all_kind_ticks(sps, ticks):
    """the ticks on which all four kinds are active"""
    return [t for t, occ in enumerate(ticks) if kinds_active(sps, occ) == set(KINDS)]


def counting_ticks(sps, ticks, admitted):
    """all-kind ticks on which an SDE request and an inpainting request stand at a stage that owns a table row (not at the
    DENOISE stage of denoise_to_zero, which is launched on its own): the first and the last of them"""
    def rowed(kind, t, occ):
        return any(sps[j]["kind"] == kind and t - admitted[j] < sps[j]["kw"]["steps"] for j in set(occ.values()))
    good = [t for t in all_kind_ticks(sps, ticks) if rowed("sde", t, ticks[t]) and rowed("blend", t, ticks[t])]
    return [good[0], good[-1]] if len(good) >= 2 else []


def expected_launches(pool):
    """the stage launches of the tick the pool is about to make (call it once the tick has admitted), by the grouping rule of
    a DPM_TABLE_NOISE | DPM_TABLE_BLEND call restated over the rows' stage records: every SDE row in one run, every blend row
    in one run, the other fusable rows grouped first come first grouped -- MS3 and UniPC records never share a group --, a
    table launch from 17 members on, a kernarg launch from 2, a lone launch for one; DENOISE stages on their own.
    Returns a dict: noise / blend runs, plain / UniPC table launches, kernarg launches of either family, lone launches."""
    import numpy as np
    from dpm_solver_amd import _lib as L
    rows = np.flatnonzero(pool._req >= 0)
    pos = pool._pos[rows]
    rec = pool._recs[pool._off[rows] + pos]
    slot, width = pool._bslot[rows], pool._brec.shape[1]
    blend = np.zeros(len(rows), dtype=bool)
    if width:
        blend = (slot >= 0) & (pool._brec[np.clip(slot, 0, None), np.minimum(pos, width - 1)]["flag"] != 0)
    out = dict(noise=0, blend=0, table=0, table_unipc=0, het=0, het_unipc=0, lone=0)
    waiting = []                                  # the third form (MS3 / UNIPC, or 0) of the rows of the plain kind, in row order
    for form, flags, bl in zip(rec["form"].tolist(), rec["flags"].tolist(), blend.tolist()):
        if bl:
            kind = "blend" if form in (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3) else "lone"
        elif flags & L.F_NOISE:
            kind = "noise" if form in (L.FORM_LIN1, L.FORM_TWO) else "lone"
        elif form in (L.FORM_LIN1, L.FORM_TWO, L.FORM_MS3) or (form == L.FORM_UNIPC and not flags & L.F_STORE_XC):
            waiting.append(form if form in (L.FORM_MS3, L.FORM_UNIPC) else 0)
            continue
        else:
            kind = "lone"
        if kind == "lone":
            out["lone"] += 1
        else:
            out[kind] = 1
    while waiting:
        third, count, later = 0, 0, []
        for f in waiting:
            if f and third and f != third:
                later.append(f)
            else:
                third, count = third or f, count + 1
        fam = "_unipc" if third == L.FORM_UNIPC else ""
        out["lone" if count == 1 else ("table" if count >= 17 else "het") + fam] += 1
        waiting = later
    return out


THR_SLOTS, THR_SHAPE = 8, (3, 8, 8)


def thresh_specs(n=10, per_tick=3):
    """the same in small for request_pool(slots=8, thresholding=True, sde=True): ten thresholded requests, three per tick"""
    return [dict(j=j, tick=j // per_tick, kind="plain", b=1 + 2 * (j % 3 == 1),
                 kw=dict(steps=4 + (5 * j) % 6, order=1 + (j // 2) % 3, skip_type=("time_uniform", "logSNR")[j % 4 == 0],
                         denoise_to_zero=(j % 7 == 3))) for j in range(n)]


def tensors(sps, dtype, device, ns, mask_blend, shape=SHAPE, seed=222):
    """(xs, conds, mbs) of the scenario, drawn on the CPU and moved: x_T of [b, *shape]; a (condition, unconditional condition)
    pair per request, of leading dimension b or 1; a MaskBlend per inpainting request (None for the others) -- x0 with a fixed
    noise, or intermediates; a [H,W] or a full-size mask"""
    g = torch.Generator().manual_seed(seed)
    to = lambda t: t.to(device).to(dtype)
    xs = [to(2.0 * torch.randn((sp["b"],) + shape, generator=g)) for sp in sps]
    conds = [(torch.rand(sp["b"] if j % 2 else 1, 1, generator=g).to(device),
              (torch.rand(1 if j % 3 else sp["b"], 1, generator=g) - 1.0).to(device)) for j, sp in enumerate(sps)]
    mbs = []
    for sp in sps:
        if sp["kind"] != "blend":
            mbs.append(None)
            continue
        full = (sp["b"],) + shape
        mask = to((torch.rand(full if sp["full_mask"] else shape[1:], generator=g) > 0.5).float())
        if sp["mode"] == "x0":
            mbs.append(mask_blend(ns, mask, x0=to(torch.randn(full, generator=g)), noise=to(torch.randn(full, generator=g))))
        else:
            mbs.append(mask_blend(ns, mask, intermediates=[to(torch.randn(full, generator=g))
                                                           for _ in range(sp["kw"]["steps"] + 2)]))
    return xs, conds, mbs


def submit(pool, sp, x, cond, mb, cfg):
    ckw = dict(condition=cond[0], unconditional_condition=cond[1]) if cfg else {}
    if sp["kind"] == "unipc":
        return pool.submit_unipc(x, **sp["kw"], **ckw)
    if sp["kind"] == "sde":
        return pool.submit(x, sde=True, **sp["kw"], **ckw)
    return pool.submit(x, blend=mb, **sp["kw"], **ckw)


def alone(solver, sp, x, cond, mb, cfg):
    """the request on its own: `solver(cond, uncond, cxt)` builds the solver of the conditions expanded to the request's b"""
    cs = [c.expand(sp["b"], -1) for c in cond] if cfg else [None, None]
    dpm = solver(cs[0], cs[1], mb)
    if sp["kind"] == "unipc":
        return dpm.sample_unipc(x, **sp["kw"])
    if sp["kind"] == "sde":
        return dpm.sample_sde(x, **sp["kw"])
    return dpm.sample(x, **sp["kw"])


def run(pool, sps, xs, conds, mbs, cfg, each_tick=None, around_step=None):
    """submit and step until the pool drains.  Per tick, `around_step(tick, step)` (default: call it) runs the step, then
    `each_tick(tick, occ, info)` sees {row: j} of the rows that tick advanced and info = dict(expect=expected_launches of the
    tick, admitted=requests the tick admitted, copies=host-to-device copies it issued).
    Returns ({j: result}, the ticks' {row: j})."""
    handles, got, ticks, tick = {}, {}, [], 0
    while tick <= max(sp["tick"] for sp in sps) or pool:
        for sp in sps:
            if sp["tick"] == tick:
                handles[submit(pool, sp, xs[sp["j"]], conds[sp["j"]], mbs[sp["j"]], cfg)] = sp["j"]
        box = {}

        def step():
            # the rows this tick advances: those active once the step has admitted, read before it frees the finished ones
            admit, waiting, copies = pool._admit, len(pool._wait), pool.copies

            def spy():
                out = admit()
                box["occ"] = {int(r): handles[int(h)] for r, h in enumerate(pool._req) if h >= 0}
                box["info"] = dict(expect=expected_launches(pool), admitted=waiting - len(pool._wait))
                return out
            pool._admit = spy
            try:
                box["done"] = pool.step()
            finally:
                del pool._admit
            box["info"]["copies"] = pool.copies - copies
        (around_step or (lambda t, f: f()))(tick, step)
        for h, out in box["done"].items():
            got[handles[h]] = out
        ticks.append(box["occ"])
        if each_tick:
            each_tick(tick, ticks[-1], box["info"])
        tick += 1
    return got, ticks
