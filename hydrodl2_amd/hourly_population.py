"""Population evaluation of `Hbv_2_hourly` at its gages: `hourly_population_stats` (`Hbv_2_hourly.population_stats`).

The hourly model's output is gage streamflow, and gages couple the units, so a unit has no score and the one-launch
shape of `population_stats` does not carry over: the call has two stages and one intermediate series.  The module runs
ONCE at `parameters`; then, per chunk of candidates,
  stage 1  hbvx_hourly_population_runoff: every candidate's hourly unit runoff [P,T,U] (the recurrence with the
           candidate's static values, the module's Qs) -- skipped when only routing parameters move;
  stage 2  hbvx_gage_population_stats: the candidates' pair hydrographs, the routing of every candidate's runoff to the
           gages in hbvx_gage_route_forward's operation order without a per-pair series, period means on one calendar and
           the four chains of `population_stats` per (candidate, gage)
(include/hbvx_gage_pop.h states both line by line).  `population_score` works on the result unchanged.

Candidates come in two families: `candidates`, columns of the static physical parameters per unit, and
`distr_candidates`, route_a / route_b / route_tau per (gage, unit) pair -- a family that only a search reaches.  The
generic `population_*` calls keep refusing the model.  hourly_events.py builds on this call: flood-event statistics of
every candidate at the gages, and the routing-only search (`hourly_routing_search`), which is separable per gage;
hourly_fdc.py does too: every candidate's flow-duration curve at the gages, counted and sorted on the device.  Not
built: a search over the unit parameters (gages share units: there is no per-gage selection), a second observed series,
cache_states, the per-unit 72-tap routing, per-gage calendars, and everything for Hbv_2_mts.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .population import _calendar, _check_rows, _observations, _period_days
from .sensitivity import direction_chunks

EXPORTS = ('hbvx_hourly_population_runoff', 'hbvx_gage_population_stats', 'hbvx_gage_population_workspace_bytes')
WHAT = "hourly_population_stats"


class _Gages(NamedTuple):
    """What population._observations and _check_rows read of a request, with the gages in the place of the basins."""
    T_out: int
    B: int


def _static_names(model) -> list:
    dyn = set(model.dynamic_params)
    return [n for n in model.parameter_bounds if n not in dyn]


def _check_names(model, names) -> list:
    static = _static_names(model)
    names = list(static if names is None else names)
    if not names:
        raise ValueError(f"{WHAT} needs at least one name")
    if len(set(names)) != len(names):
        raise ValueError(f"{WHAT}: a name is listed twice in {names}")
    for n in names:
        if n in model.dynamic_params:
            raise ValueError(f"{WHAT}: {n} is a dynamic parameter of this model (its values come from p_dyn, hour by hour); "
                             "only static parameters have candidates")
        if n not in static:
            raise ValueError(f"{WHAT}: unknown parameter name {n!r}; the static physical parameters are {static}")
    return names


def hourly_population_columns(model, names: Optional[Sequence[str]] = None) -> list:
    """The columns of `p_sta` that `hourly_population_stats(..., candidates, names=names)` stands in for: nmul columns per
    static physical parameter of `names`, in that order (default: every parameter of parameter_bounds that is not
    dynamic).  What `jacobian_columns` is to the daily models."""
    if getattr(model, '_model_id', None) != _abi.MODEL_HOURLY:
        raise NotImplementedError(f"hourly_population_columns is for Hbv_2_hourly, not {type(model).__name__}")
    static = _static_names(model)
    M = model.nmul
    return [static.index(n) * M + j for n in _check_names(model, names) for j in range(M)]


def _check_model(model):
    if getattr(model, '_model_id', None) != _abi.MODEL_HOURLY:
        raise NotImplementedError(f"{WHAT} is for Hbv_2_hourly, not {type(model).__name__}: Hbv, Hbv_1_1p and Hbv_2 go "
                                  "through hydrodl2_amd.population_stats, HbvAdj through adj_population_stats")
    if model.graph:
        raise ValueError(f"{WHAT}: Hbv_2_hourly(graph=True) replays one captured call; use graph=False")
    if model.initialize:
        raise ValueError(f"{WHAT}: the module is in initialize mode (it returns states, no flux dictionary)")
    if model.cache_states:
        raise ValueError(f"{WHAT}: cache_states=True is not supported (the routed history is detached and spans calls: "
                         "a candidate's runoff of this call alone is not what the gages see)")
    if model.routing:
        raise ValueError(f"{WHAT}: routing=True (the optional 72-tap per-unit routing) is not supported")
    if not model.use_distr_routing:
        raise ValueError(f"{WHAT}: use_distr_routing=False leaves no gage streamflow to score")


def _check_tensor(name, t, shape_text, ok, dev):
    if not torch.is_tensor(t) or not ok(t):
        raise ValueError(f"{WHAT}: {name} must be {shape_text}, got "
                         f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{WHAT}: {name} must be float32, got {t.dtype}")
    if t.device != dev:
        raise ValueError(f"{WHAT}: {name} lives on {t.device}, x_phy on {dev}")


def _default_chunk(P, per_candidate_bytes, dev) -> int:
    """All candidates, or as many as fit into half of the free device memory."""
    if dev.type != 'cuda':
        return P
    free, _ = torch.cuda.mem_get_info(dev)
    return max(1, min(P, int((free // 2) // max(per_candidate_bytes, 1))))


def hourly_population_stats(model, x_dict: dict, parameters, target, candidates: Optional[torch.Tensor] = None,
                            distr_candidates: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None,
                            weights=None, periods=None, transform: str = 'none', eps=None, return_series: bool = False,
                            max_candidates: Optional[int] = None) -> dict:
    """The sums from which `population_score` forms NSE, KGE, correlation, variability and bias of gage streamflow for
    each of P candidate parameter sets of `Hbv_2_hourly`, on one run of the module.

    candidates        [P,U,C] float32 or None: unit-interval values for the columns
                      `hourly_population_columns(model, names)` returns, in that order.  Candidate c stands in for
                      p_sta[u, columns]; dynamic parameters, the other columns, forcings and muwts are shared.
    distr_candidates  [P,n_pairs,3] float32 or None: unit-interval route_a, route_b, route_tau per (gage, unit) pair in
                      the pair order of `GageTopology` (by gage, then unit); candidate c stands in for parameters[2].
                      At least one of the two; with both, candidate c is the pair (candidates[c], distr_candidates[c]).
    target            [K,G] or [K,G,1]: gage streamflow in the module's units per period; NaN is a missing observation.
    weights           [K,G] >= 0 or None (ones).
    periods           None: every hour its own period (K = T); an int n: blocks of n hours, an incomplete last block is
                      not scored; an ascending sequence of closing hours.  With a calendar the gage series is averaged
                      over each period before it meets its target -- hourly simulations against daily-mean gauge records
                      are periods=24.  Hours after the last closing hour are simulated and not scored.  The calendar
                      and row checks are `population_period_stats`' own, unchanged, so their messages speak of "days per
                      period" and "closing days" where this call's steps are hours.
    transform, eps    as `population_stats`, with shift and eps per gage.
    max_candidates    at most so many candidates in flight (bounds the scratch: [P,T,U] runoff twice, [P,T,G], the
                      candidates' taps); default: all, or what fits into half of the free device memory.  The primal is
                      never split, and a candidate's bits do not depend on the split.
    Returns `population_stats`' dictionary with gages for basins: 'sse', 's1', 's2', 's3' [P,G] float32 (as the kernel
    wrote them: a non-finite sum is not replaced), 'shift', 'obs', 'transform', 'eps', 'n_obs' [G], 'columns' (the p_sta
    columns, [] without `candidates`), 'outputs' (the primal dictionary of the one module run); with a calendar also
    'period_ends' and 'period_days'; with return_series 'series' [P,K,G], the period means (not their transform).

    The module runs once at `parameters`: that run draws the dy_drop masks -- one set, shared by all candidates -- and
    leaves the module as one plain call does.  Two calls agree bit for bit; the hourly gage series of a candidate has the
    bits of the module's own gage routing on that candidate's runoff and routing parameters.

    Refused before the model runs: any other model (NotImplementedError); graph=True, initialize mode,
    cache_states=True, routing=True, use_distr_routing=False, dynamic or unknown names, a wrong shape / dtype / device of
    any tensor, infinite targets, negative or non-finite weights, a calendar `population_period_stats` would refuse,
    max_candidates < 1 (ValueError); a library without the exports (HbvxError naming the missing one)."""
    return _evaluate(model, x_dict, parameters, target, candidates, distr_candidates, names, weights, periods, transform,
                     eps, return_series, max_candidates)


def _evaluate(model, x_dict, parameters, target, candidates, distr_candidates, names, weights, periods, transform, eps,
              return_series, max_candidates, hook=None) -> dict:
    """The body of `hourly_population_stats`, and of the calls that want more of a chunk's hourly gage series than its
    four sums (hourly_events.py, hourly_fdc.py).  `hook`, if given, has
      check(T, G, dev)   the caller's own refusals, after this call's and before the library is asked or the model runs;
      exports            the exports it needs beyond EXPORTS;
      bytes              what it writes per candidate;
      chunk(series)      called once per chunk of candidates with that chunk's [p,T,G] series, before the next chunk
                         overwrites the scratch the series came with.
    Without a hook the series stays in the export's own scratch, and the launches are what they were."""
    _check_model(model)
    x = x_dict['x_phy']
    dev = x.device
    T, U = int(x.shape[0]), int(x.shape[1])
    topo = x_dict['outlet_topo']
    G = int(topo.shape[0])
    if candidates is None and distr_candidates is None:
        raise ValueError(f"{WHAT} needs candidates, distr_candidates or both")
    if max_candidates is not None and max_candidates < 1:
        raise ValueError(f"{WHAT}: max_candidates must be >= 1")
    cols, sources = [], {}
    if candidates is not None:
        names = _check_names(model, names)
        cols = hourly_population_columns(model, names)
        C = len(cols)
        _check_tensor("candidates", candidates, f"[P,{U},{C}] (P >= 1 sets for the {C} columns of `names`)",
                      lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (U, C) and t.shape[0] >= 1, dev)
        sources = {_abi.PARAM_SLOTS.index(n): i * model.nmul for i, n in enumerate(names)}
    elif names is not None:
        raise ValueError(f"{WHAT}: names without candidates")
    n_pair = int((topo == 1).sum())
    if distr_candidates is not None:
        _check_tensor("distr_candidates", distr_candidates, f"[P,{n_pair},3] (P >= 1 sets for the {n_pair} pairs of outlet_topo)",
                      lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (n_pair, 3) and t.shape[0] >= 1, dev)
        if candidates is not None and int(candidates.shape[0]) != int(distr_candidates.shape[0]):
            raise ValueError(f"{WHAT}: candidates hold {int(candidates.shape[0])} sets, distr_candidates "
                             f"{int(distr_candidates.shape[0])}")
    P = int((candidates if candidates is not None else distr_candidates).shape[0])
    gages = _Gages(T, G)
    ends = _calendar(periods, T, "periods", WHAT)
    K = int(ends.numel())
    _check_rows(gages, x_dict, target, weights, K, f"{K} periods of its calendar" if periods is not None else "hours of the record",
                WHAT)
    ob = _observations(gages, x_dict, target, weights, transform, eps, WHAT, rows=K)
    if hook is not None:
        hook.check(T, G, dev)
    lib = get_library()
    for name in EXPORTS + (() if hook is None else tuple(hook.exports)):
        lib.require(name)

    with torch.no_grad(), ops.record_paths() as records, ops.record_gage_routes() as routes:
        outputs = model(x_dict, parameters)
    main, grec = records[-1], routes[-1]
    if main.cfg.T != T or main.cfg.B != U or grec.topo.T != T or grec.topo.G != G or grec.topo.n_pair != n_pair:
        raise RuntimeError(f"Hbv_2_hourly ran {main.cfg.T} hours on {main.cfg.B} units to {grec.topo.G} gages, expected "
                           f"{T} on {U} to {G}")
    term = ops.PopTerm(ob['target'], ob['w'], ob['shift'], ob['eps'], transform)
    ends_dev = ends.to(device=dev, dtype=torch.int32)
    cands = None if candidates is None else candidates.detach().contiguous()
    dcands = None if distr_candidates is None else distr_candidates.detach().contiguous()
    per = 4 * ((2 * T * U if cands is not None else 0) + T * G + (n_pair * min(T, _abi.GAGE_MAXLEN) if dcands is not None else 0)
               + (K * G if return_series else 0))
    if hook is not None:
        per += 4 * T * G + int(hook.bytes)      # the [p,T,G] series is then an output of its own, beside the scratch
    chunk = max_candidates or _default_chunk(P, per, dev)
    parts = []
    for c0, c1 in direction_chunks(P, chunk):
        if cands is not None:
            piece = cands[c0:c1]
            runoff = ops.hourly_population_runoff(main, {slot: (piece, col) for slot, col in sources.items()}, c1 - c0)
        else:
            runoff = grec.qs            # the primal run's own [T,U] runoff serves every candidate
        got = ops.gage_population(grec, runoff, None if dcands is None else dcands[c0:c1], term, ends_dev, return_series,
                                  want_gage=hook is not None)
        parts.append(got[:5])
        if hook is not None:
            hook.chunk(got[5])
    got = [None if parts[0][i] is None else (parts[0][i] if len(parts) == 1 else torch.cat([p[i] for p in parts]))
           for i in range(5)]
    out = dict(zip(('sse', 's1', 's2', 's3'), got[:4]))
    out.update(shift=ob['shift'], obs=ob['obs'], transform=transform, eps=ob['eps'], n_obs=ob['n_obs'], columns=cols,
               outputs=outputs)
    if periods is not None:
        out.update(period_ends=ends.clone(), period_days=_period_days(ends))
    if return_series:
        out['series'] = got[4]
    return out
