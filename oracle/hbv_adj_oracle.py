"""hbv_adj_oracle.py -- CPU ORACLE for the implicit HBV ("HBV adjoint").  TEST INFRASTRUCTURE ONLY.

A float64 torch-on-CPU restatement of the algorithm the reference's `HbvAdj` specifies
(src/hydrodl2/models/hbv/hbv_adj.py), vectorised over lanes, looping over days (small cases).

PARITY UNPINNED: the reference file cannot be imported (it needs the encrypted
`batch_jacobian.pye` and has the defects listed in SURVEY.md §2 #13) and the reference's tests skip
it (tests/test_methods.py:26-27), so there is nothing to pin this oracle against.  What it provides
instead is independence from the product: the forward follows the reference text line by line and
the gradients come from **autograd**, not from the hand-derived adjoint of
hydrodl2_amd/csrc/hbv_adj_step.h:
  after the Newton loop has produced x (no grad), one extra Newton step is taken with the Jacobian
  detached, x' = x - J(x)^-1 G(x; theta_t, x_t); then dx'/dtheta = -J^-1 dG/dtheta and
  dx'/dx_t = J^-1/dt, i.e. exactly the implicit-function derivative of hbv_adj.py:617-633, while
  the VALUE passed on is x itself.

`stop='lane'` evaluates the stopping rule per (basin, member) as the product does;
`stop='global'` is the reference's rule (one `torch.max` over the batch, hbv_adj.py:544).
"""
from __future__ import annotations

import torch

BOUNDS = {  # hbv_adj.py:59-76,94-95
    'parBETA': [1.0, 6.0], 'parFC': [50, 1000], 'parK0': [0.05, 0.9], 'parK1': [0.01, 0.5],
    'parK2': [0.001, 0.2], 'parLP': [0.2, 1], 'parPERC': [0, 10], 'parUZL': [0, 100],
    'parTT': [-2.5, 2.5], 'parCFMAX': [0.5, 10], 'parCFR': [0, 0.1], 'parCWH': [0, 0.2],
    'parBETAET': [0.3, 5],
}
NAMES12 = list(BOUNDS)[:12]


def fluxes(y, theta, clim, names):
    """hbv_adj.py:385-498: the clamped storages, the potentials and every flux of the right-hand side, by name, from
    storages y [N,5] and unit parameters theta [N,n]."""
    P = {n: BOUNDS[n][0] + theta[:, i] * (BOUNDS[n][1] - BOUNDS[n][0]) for i, n in enumerate(names)}
    SNOWPACK = torch.clamp(y[:, 0], min=0.0)   # :387-391
    MELTWATER = torch.clamp(y[:, 1], min=0.0)
    SM = torch.clamp(y[:, 2], min=1e-8)
    SUZ = torch.clamp(y[:, 3], min=0.0)
    SLZ = torch.clamp(y[:, 4], min=0.0)
    Pr, T, Ep = clim[:, 0], clim[:, 1], clim[:, 2]
    TT, CFMAX, CFR = P['parTT'], P['parCFMAX'], P['parCFR']
    sf = Pr * (T < TT)                                                          # :444-446
    rpot = torch.clamp(CFR * CFMAX * (TT - T), min=0.0)
    refr = torch.min(rpot, MELTWATER)                                           # :448-452
    mpot = torch.clamp(CFMAX * (T - TT), min=0.0)
    melt = torch.min(mpot, SNOWPACK)                                            # :454-458
    rf = Pr * (T >= TT)                                                         # :460-462
    Isnow = torch.clamp(MELTWATER - P['parCWH'] * SNOWPACK, min=0.0)            # :464-468
    sw = torch.clamp((SM / P['parFC']) ** P['parBETA'], min=0.0, max=1.0)       # :470-474
    Peff = (rf + Isnow) * sw
    ex = torch.clamp(SM - P['parFC'], min=0.0)                                  # :476-479
    ef0 = SM / (P['parLP'] * P['parFC'])                                        # :481-486
    if 'parBETAET' in P:
        ef0 = ef0 ** P['parBETAET']
    ef = torch.clamp(ef0, min=0.0, max=1.0)
    pe = Ep * ef
    et = torch.min(SM, pe)
    perc = torch.min(SUZ, P['parPERC'])                                         # :492-494
    q0 = P['parK0'] * torch.clamp(SUZ - P['parUZL'], min=0.0)                   # :488-490
    q1 = P['parK1'] * SUZ                                                       # :496-498
    q2 = P['parK2'] * SLZ
    return dict(SNOWPACK=SNOWPACK, MELTWATER=MELTWATER, SM=SM, SUZ=SUZ, SLZ=SLZ, sf=sf, rf=rf, rpot=rpot, refr=refr,
                mpot=mpot, melt=melt, Isnow=Isnow, Peff=Peff, ex=ex, ef0=ef0, pe=pe, et=et, perc=perc, q0=q0, q1=q1,
                q2=q2, y2=y[:, 2], warm=T > TT, T=T, TT=TT, CFMAX=CFMAX, CFR=CFR, FC=P['parFC'], PERC=P['parPERC'],
                UZL=P['parUZL'])


def rhs(y, theta, clim, names):
    """hbv_adj.py:341-442: dS [N,5] and Q [N] from storages y [N,5], unit parameters theta [N,n]."""
    f = fluxes(y, theta, clim, names)
    dS = torch.stack([f['sf'] + f['refr'] - f['melt'],                          # :425-429
                      f['melt'] - f['refr'] - f['Isnow'],
                      f['Isnow'] + f['rf'] - f['Peff'] - f['ex'] - f['et'],
                      f['Peff'] + f['ex'] - f['perc'] - f['q0'] - f['q1'],
                      f['perc'] - f['q2']], dim=1)
    return dS, f['q0'] + f['q1'] + f['q2']                                      # :431


def branches(y, theta, clim, names):
    """Which side of every min / max / threshold of the right-hand side the state y [N,5] lies on: name -> bool [N].
    A limited flux counts only where it flows (melt limited by a pack that is there, and so on)."""
    with torch.no_grad():
        f = fluxes(y, theta, clim, names)
        wet, q0a = f['SM'] > f['FC'], f['SUZ'] > f['UZL']
        lin = f['SUZ'] <= f['PERC']                                             # perc = SUZ
        return {
            'rain': f['rf'] > 0, 'snow': f['sf'] > 0,
            'melt_pack_limited': (f['melt'] > 0) & (f['SNOWPACK'] < f['mpot']),
            'melt_potential': (f['melt'] > 0) & (f['SNOWPACK'] > f['mpot']),
            'refr_mw_limited': (f['refr'] > 0) & (f['MELTWATER'] < f['rpot']),
            'refr_potential': (f['refr'] > 0) & (f['MELTWATER'] > f['rpot']),
            'isnow_warm': (f['Isnow'] > 0) & f['warm'], 'isnow_cold': (f['Isnow'] > 0) & ~f['warm'],
            'sm_above_fc': wet, 'sm_below_fc': ~wet,
            'ef_clamped': f['ef0'] > 1, 'ef_free': f['ef0'] <= 1,
            'et_sm_limited': f['SM'] < f['pe'], 'et_pet_limited': f['SM'] >= f['pe'],
            'sm_floor': f['y2'] < 1e-8,
            'perc_suz': lin, 'perc_par': ~lin, 'q0_active': q0a, 'q0_idle': ~q0a,
            'gw_suz_idle': lin & ~q0a, 'gw_suz_q0': lin & q0a, 'gw_par_idle': ~lin & ~q0a, 'gw_par_q0': ~lin & q0a,
        }


def _G(x, theta, xt, clim, names, dt=1.0):
    """hbv_adj.py:669-678 (backward Euler)."""
    f, _ = rhs(x, theta, clim, names)
    return (x - xt) / dt - f


def _jac(x, theta, xt, clim, names):
    """Batched dG/dx [N,5,5] by autograd (what the reference's batchJacobian is used for)."""
    with torch.enable_grad():
        xx = x.detach().requires_grad_(True)
        g = _G(xx, theta.detach(), xt.detach(), clim, names)
        rows = [torch.autograd.grad(g[:, i].sum(), xx, retain_graph=True)[0] for i in range(5)]
    return torch.stack(rows, dim=1)


def newton_day(theta, xt, clim, names, gtol=1e-3, max_iter=3, stop='lane'):
    """hbv_adj.py:507-581.  Returns x [N,5] (no grad) and the update count per lane."""
    with torch.no_grad():
        x = xt.detach().clone()
        th = theta.detach()
        g = _G(x, th, xt.detach(), clim, names)
        J = _jac(x, th, xt, clim, names)
        res = g.abs().amax(dim=1)
        res0 = 100 * res
        it = torch.zeros_like(res)
        i = 0
        while True:
            if stop == 'global':
                active = torch.full_like(res, bool((res.max() > gtol) and i <= max_iter), dtype=torch.bool)
            else:
                active = (res > gtol) & (it <= max_iter)
            if not bool(active.any()):
                break
            i += 1
            it = it + active.to(it.dtype)
            refresh = active & (res > 0.2 * res0) if stop == 'lane' \
                else active & bool((res / res0).max() > 0.2)
            if bool(refresh.any()):
                Jn = _jac(x, th, xt, clim, names)
                J = torch.where(refresh[:, None, None], Jn, J)
            dx = torch.linalg.solve(J, g.unsqueeze(-1)).squeeze(-1)
            x = torch.where(active[:, None], x - dx, x)
            gn = _G(x, th, xt.detach(), clim, names)
            resn = gn.abs().amax(dim=1)
            res0 = torch.where(active, res, res0)
            res = torch.where(active, resn, res)
            g = torch.where(active[:, None], gn, g)
    return x, it


def implicit_step(theta, xt, clim, names, **kw):
    """One day with implicit-function gradients (see module docstring)."""
    x, it = newton_day(theta, xt, clim, names, **kw)
    J = _jac(x, theta, xt, clim, names)
    g = _G(x, theta, xt, clim, names)                       # differentiable in theta and xt
    xnew = x - torch.linalg.solve(J, g.unsqueeze(-1)).squeeze(-1)
    return x + (xnew - xnew.detach()), it                   # value x, gradient of xnew


def uh_gamma(a, b, L):
    """core/calc/uh_routing.py:5-22 for a,b [B]."""
    aa = torch.relu(a) + 0.1
    theta = torch.relu(b) + 0.5
    t = torch.arange(0.5, L * 1.0, dtype=a.dtype)[:, None]
    w = 1 / (aa.lgamma().exp() * theta ** aa) * t ** (aa - 1) * torch.exp(-t / theta)
    return w / w.sum(0)                                     # [L,B]


def uh_conv(q, w):
    """core/calc/uh_routing.py:25-57: y[t,b] = sum_k w[k,b] q[t-k,b]."""
    T, L = q.shape[0], w.shape[0]
    y = torch.zeros_like(q)
    for k in range(min(L, T)):
        y[k:] = y[k:] + w[k] * q[:T - k]
    return y


def lane_inputs(x_phy, parameters, nmul=1, warm_up=0, dynamic_params=(), dy_drop=0.0, routing=True,
                dtype=torch.float64):
    """hbv_adj.py:133-196,261-262: what every day of the run works on, in the member-major lane order (lane j*B + b).
    Returns names, the warm-up pass's unit parameters [warm_up,N,n] (None without one), the main pass's [T',N,n] (the
    dy_drop masks are drawn here, from the default generator), the forcing [T,N,3] and the routing parameters."""
    names = list(NAMES12) + (['parBETAET'] if 'parBETAET' in dynamic_params else [])
    n = len(names)
    T, B = x_phy.shape[0], x_phy.shape[1]
    N = B * nmul
    x_phy = x_phy.to(dtype)
    par = parameters.to(dtype)
    # :133-147 member-major lanes
    phy = torch.sigmoid(par[:, :, :n * nmul]).view(T, B, n, nmul).permute(0, 3, 1, 2).reshape(T, N, n)
    rout = torch.sigmoid(par[-1, :, n * nmul:]) if routing else None

    def make(phy_slice, dy_list):                           # :156-196
        nt = phy_slice.shape[0]
        sta = phy_slice[-1].unsqueeze(0).repeat(nt, 1, 1)
        if not dy_list:
            return sta
        full = sta.clone()
        pmat = torch.ones([1, N]) * dy_drop
        cols = []
        for i, name in enumerate(names):
            if name in dy_list:
                dr = torch.bernoulli(pmat).to(dtype)
                cols.append(phy_slice[:, :, i] * (1 - dr) + sta[:, :, i] * dr)
            else:
                cols.append(full[:, :, i])
        return torch.stack(cols, dim=2)

    clim = x_phy.unsqueeze(1).repeat(1, nmul, 1, 1).view(T, N, 3)   # :261-262,285-286
    pw = make(phy[:warm_up], []) if warm_up > 0 else None           # :257-274
    pr = make(phy[warm_up:], list(dynamic_params))
    return names, pw, pr, clim, rout


def hbv_adj_forward(x_phy, parameters, nmul=1, warm_up=0, dynamic_params=(), dy_drop=0.0,
                    gtol=1e-3, max_iter=3, stop='lane', routing=True, dtype=torch.float64, y0=None, events=None):
    """hbv_adj.py:227-330.  x_phy [T,B,3], raw parameters [T,B,ny] -> flow_sim [T',B,1]
    (differentiable w.r.t. `parameters`); also returns the Newton update counts [T',N].

    y0      [N,5]: the storages the run starts from (the warm-up pass, if there is one), in the member-major lane
            order, differentiable; None: zeros (hbv_adj.py:254).
    events  a dict: receives name -> bool [T',N], the branches of the right-hand side taken at the solved state of
            every day of the main pass (`branches`)."""
    T, B = x_phy.shape[0], x_phy.shape[1]
    N = B * nmul
    names, pw, pr, clim, rout = lane_inputs(x_phy, parameters, nmul, warm_up, dynamic_params, dy_drop, routing, dtype)
    y = torch.zeros((N, 5), dtype=dtype) if y0 is None else y0.to(dtype)    # :254
    kw = dict(gtol=gtol, max_iter=max_iter, stop=stop)
    for t in range(warm_up):                                        # :257-274
        y, _ = implicit_step(pw[t], y, clim[t], names, **kw)
    nt = T - warm_up
    sims, its, evs = [], [], []
    for t in range(nt):                                             # :689-712, :309-313
        y, it = implicit_step(pr[t], y, clim[warm_up + t], names, **kw)
        _, Q = rhs(y, pr[t], clim[warm_up + t], names)
        sims.append(Q)
        its.append(it)
        if events is not None:
            evs.append(branches(y, pr[t], clim[warm_up + t], names))
    if events is not None:
        events.update({k: torch.stack([e[k] for e in evs]) for k in evs[0]})
    sim = torch.stack(sims).view(nt, nmul, B).mean(dim=1)           # :315-317
    if routing:
        a = rout[:, 0] * 2.9
        b = rout[:, 1] * 6.5
        sim = uh_conv(sim, uh_gamma(a, b, min(nt, 15)))             # :319-325
    return sim.unsqueeze(-1), torch.stack(its)
