"""Plain-torch float64 references of adaptive projected guidance (Sadat et al. 2024) -- TEST INFRASTRUCTURE, never imported by
the product, and importing nothing of it: no planner, no wrapper, no kernel double.

`ApgModel64` is the guided model function written out: it calls a `raw(x, t) -> (conditional, unconditional)` pair of raw
network outputs, forms the two data predictions, the direction, its running average (the object's own state: one object per
run, one call per network evaluation, in order), the norm cap, the projection and the guided data prediction, all in float64,
and returns the equivalent noise prediction.  `torch_2m_float64` is DPM-Solver++(2M) written out around such a function."""
import torch


class ApgModel64:
    def __init__(self, raw, ns, model_type, scale, eta, r, beta):
        self.raw, self.ns, self.model_type = raw, ns, model_type
        f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))      # the stage record carries fp32 scalars
        self.scale, self.eta, self.r, self.beta = f32(scale), f32(eta), f32(r), f32(beta)
        self.avg = None

    def x0(self, x, t):
        """the guided data prediction at (x, t[B]); updates the running average"""
        x = x.double()
        shp = (-1,) + (1,) * (x.dim() - 1)
        a = self.ns.marginal_alpha(t.double().cpu()).reshape(shp).to(x.device)
        s = self.ns.marginal_std(t.double().cpu()).reshape(shp).to(x.device)
        e0, e1 = (o.double() for o in self.raw(x, t))

        def x0_of(o):
            eps = {"noise": lambda: o, "x_start": lambda: (x - a * o) / s, "v": lambda: a * o + s * x,
                   "score": lambda: -s * o}[self.model_type]()
            return (x - s * eps) / a
        c = x0_of(e0)
        d = c - x0_of(e1)
        if self.beta != 0.0:
            self.avg = d + self.beta * (self.avg if self.avg is not None else torch.zeros_like(d))
            d = self.avg
        axes = list(range(1, x.dim()))
        s_dd, s_dc, s_cc = ((u * v).sum(dim=axes, keepdim=True) for u, v in ((d, d), (d, c), (c, c)))
        sc = torch.ones_like(s_dd)
        if self.r > 0.0:
            sc = torch.clamp(self.r / s_dd.sqrt(), max=1.0)
        dn, par = sc * d, (sc * s_dc / s_cc) * c
        return c + (self.scale - 1.0) * ((dn - par) + self.eta * par), a, s

    def __call__(self, x, t):
        x0, a, s = self.x0(x, t)
        return (x.double() - a * x0) / s


def torch_2m_float64(model_fn, ns, x, steps):
    """DPM-Solver++(2M) in torch float64: the reference's multistep loop (ref :1171-1212) with time_uniform steps,
    lower_order_final, solver_type 'dpmsolver' (ref :547-592, :827-851).  model_fn(x, t_continuous[B]) -> noise, called once
    per step in trajectory order; the schedule's marginals are evaluated at double times."""
    dev, B = x.device, x.shape[0]
    ts = torch.linspace(ns.T, 1. / ns.total_N, steps + 1).double()                      # the reference's fp32 grid, exactly
    marg = lambda t: tuple(float(f(t.reshape(1))) for f in (ns.marginal_lambda, ns.marginal_alpha, ns.marginal_std))

    def x0_at(xx, t):                                                                   # data_prediction_fn, ref :433-442
        _, a, s = marg(t)
        return (xx - s * model_fn(xx, t.to(dev).expand(B)).double()) / a
    x = x.double()
    hist, t_hist = [x0_at(x, ts[0])], [ts[0]]
    for i in range(1, steps + 1):
        order = 1 if i == 1 or i == steps else 2                                        # warm-up; lower_order_final (steps < 10)
        lam_t, a_t, s_t = marg(ts[i])
        lam_0, _, s_0 = marg(t_hist[-1])
        h = lam_t - lam_0
        phi_1 = torch.expm1(torch.tensor(-h, dtype=torch.float64)).item()
        x_t = (s_t / s_0) * x - (a_t * phi_1) * hist[-1]
        if order == 2:
            r0 = (lam_0 - marg(t_hist[-2])[0]) / h
            x_t = x_t - 0.5 * (a_t * phi_1) * ((1. / r0) * (hist[-1] - hist[-2]))
        x = x_t
        if i < steps:
            hist, t_hist = (hist + [x0_at(x, ts[i])])[-2:], (t_hist + [ts[i]])[-2:]
    return x
