"""HBV with an implicit (backward-Euler) time step and an implicit-function adjoint.

Counterpart of the reference's `HbvAdj` (src/hydrodl2/models/hbv/hbv_adj.py:15-330).  The
reference file cannot be imported (it needs an encrypted dependency and has several defects,
SURVEY.md §2 #13); this class implements the algorithm that file specifies:

* per day solve  G(x) = (x - x_t)/dt - f(x, theta_t, t) = 0  (hbv_adj.py:669-678) with the
  flux-form right-hand side of hbv_adj.py:385-431, by modified Newton (<= 4 updates, gtol 1e-3 on
  |G|_inf, Jacobian refreshed when the residual ratio exceeds 0.2: hbv_adj.py:516-581);
* streamflow = ensemble mean of q0+q1+q2 at the solved states (hbv_adj.py:309-317), routed with the
  gamma unit hydrograph (hbv_adj.py:319-325); only `flow_sim` is returned (hbv_adj.py:328-330);
* backward = implicit-function adjoint (hbv_adj.py:617-633).

Same constructor / config keys / attributes as the reference (`rout_a`, `rout_b` routing names,
`ad_efficient` accepted and ignored).  Differences, all deliberate:
  - the Newton stopping rule is per (basin, member), not one maximum over the whole batch;
  - `parBETAET` is used only when it is listed dynamic (its bounds exist only then,
    hbv_adj.py:94-95); the reference reads it unconditionally and would raise KeyError;
  - derivatives are analytic (the reference mixes an autograd Jacobian with float64 finite
    differences, hbv_adj.py:531,606).
"""
from typing import Any, Optional

import torch

from hydrodl2_amd import _abi
from hydrodl2_amd.ops import HbvAdjPath, ParamSource, RouteSource, StepConfig, has_tangent


class HbvAdj(torch.nn.Module):
    """HBV adjoint: 12 (+parBETAET) physical parameters x nmul, 2 routing parameters."""

    def __init__(self, config: Optional[dict[str, Any]] = None,
                 device: Optional[torch.device] = None) -> None:
        super().__init__()
        # hbv_adj.py:46-76
        self.name = 'HBV Adjoint'
        self.config = config
        self.initialize = False
        self.warm_up = 0
        self.dynamic_params = []
        self.dy_drop = 0.0
        self.variables = ['prcp', 'tmean', 'pet']
        self.routing = True
        self.comprout = False
        self.nearzero = 1e-5
        self.nmul = 1
        self.ad_efficient = True
        self.device = device
        self.newton_gtol = 1e-3      # hbv_adj.py:519
        self.newton_max_iter = 3     # hbv_adj.py:518
        # 'lane': every (basin, member) stops for itself; 'global': the reference's rule (hbv_adj.py:544,546:
        # one torch.max over the batch) applied to the 64 lanes of a wavefront (include/hbvx.h, adj_stop)
        self.newton_stop = 'lane'
        # 'staged' (default): the block lower-triangular system is solved block by block -- snow, upper and lower
        # zone in closed form, soil moisture by scalar Newton under newton_gtol / newton_max_iter (csrc/hbv_adj_step.h
        # AdjStaged; the three blocks run as a wave pipeline).  'joint': the reference's modified Newton on all five
        # unknowns (hbv_adj.py:507-581), kept as the policy cross-check; newton_stop applies to it only.
        self.newton_solver = 'staged'
        self.graph = False           # replay the call's launches as HIP graphs (hydrodl2_amd/graphed.py); opt-in
        self.grad_buffer = 'fresh'   # 'persistent': the [T,B,ny] gradient in a buffer kept per shape (core/hbv_module.py)
        self._cfg_cache = {}
        self._memo_cache = {}
        self.parameter_bounds = {
            'parBETA': [1.0, 6.0], 'parFC': [50, 1000], 'parK0': [0.05, 0.9],
            'parK1': [0.01, 0.5], 'parK2': [0.001, 0.2], 'parLP': [0.2, 1],
            'parPERC': [0, 10], 'parUZL': [0, 100], 'parTT': [-2.5, 2.5],
            'parCFMAX': [0.5, 10], 'parCFR': [0, 0.1], 'parCWH': [0, 0.2],
        }
        self.routing_parameter_bounds = {'rout_a': [0, 2.9], 'rout_b': [0, 6.5]}
        if not device:
            self.device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        if config is not None:  # hbv_adj.py:81-95
            self.warm_up = config.get('warm_up', self.warm_up)
            self.dy_drop = config.get('dy_drop', self.dy_drop)
            self.dynamic_params = config['dynamic_params'].get(
                self.__class__.__name__, self.dynamic_params)
            self.variables = config.get('variables', self.variables)
            self.routing = config.get('routing', self.routing)
            self.comprout = config.get('comprout', self.comprout)
            self.nearzero = config.get('nearzero', self.nearzero)
            self.nmul = config.get('nmul', self.nmul)
            self.ad_efficient = config.get('ad_efficient', self.ad_efficient)
            self.newton_gtol = config.get('newton_gtol', self.newton_gtol)
            self.newton_max_iter = config.get('newton_max_iter', self.newton_max_iter)
            self.newton_stop = config.get('newton_stop', self.newton_stop)
            self.graph = bool(config.get('graph', self.graph))
            self.grad_buffer = config.get('grad_buffer', self.grad_buffer)
            if self.grad_buffer not in ('fresh', 'persistent'):
                raise ValueError("grad_buffer must be 'fresh' or 'persistent'")
            if self.newton_stop not in ('lane', 'global'):
                raise ValueError("newton_stop must be 'lane' or 'global'")
            # The solver never follows from the mere PRESENCE of another key: 'staged' unless asked otherwise.  The one
            # value that only the joint iteration implements -- the reference's batch-wide stopping rule -- selects it.
            self.newton_solver = config.get('newton_solver',
                                            'joint' if self.newton_stop == 'global' else self.newton_solver)
            if self.newton_solver not in ('staged', 'joint'):
                raise ValueError("newton_solver must be 'staged' or 'joint'")
            if self.newton_solver == 'staged' and self.newton_stop == 'global':
                raise ValueError("newton_stop='global' is a rule of the joint iteration: use newton_solver='joint'")
            if 'parBETAET' in self.dynamic_params:
                self.parameter_bounds['parBETAET'] = [0.3, 5]
        self.set_parameters()

    def set_parameters(self) -> None:
        """hbv_adj.py:99-109."""
        self.phy_param_names = self.parameter_bounds.keys()
        self.routing_param_names = self.routing_parameter_bounds.keys() if self.routing else []
        self.rout_params_name = list(self.routing_parameter_bounds.keys())
        self.learnable_param_count = len(self.phy_param_names) * self.nmul + len(
            self.routing_param_names)

    def _lane_drop_mask(self, ngrid: int, device) -> torch.Tensor:
        """hbv_adj.py:182-189: one Bernoulli(dy_drop) per LANE of the member-major batch
        (index j*B + b); returned in this package's basin-major lane order (b*M + j)."""
        pmat = torch.ones([1, ngrid * self.nmul]) * self.dy_drop
        drmask = torch.bernoulli(pmat)      # drawn even for dy_drop == 0: same consumption of the host generator
        if self.dy_drop <= 0:
            return None                     # nothing dropped: no mask, no host-to-device copy per call
        m = drmask.reshape(self.nmul, ngrid).t().contiguous().reshape(-1)
        return m.to(torch.uint8).to(device)

    def _advance_rng(self, ngrid: int) -> None:
        """Consume the CPU generator as one call of forward() does (one draw per dynamic parameter)."""
        for _ in self.dynamic_params:
            self._lane_drop_mask(ngrid, torch.device('cpu'))

    def _settings_key(self):
        return (self.nmul, tuple(self.parameter_bounds), tuple(self.dynamic_params), bool(self.routing),
                tuple(self.variables), float(self.nearzero), int(self.warm_up), float(self.dy_drop),
                float(self.newton_gtol), int(self.newton_max_iter), self.newton_stop, self.newton_solver,
                str(self.grad_buffer), tuple(map(tuple, self.parameter_bounds.values())),
                tuple(map(tuple, self.routing_parameter_bounds.values())))

    _graph_state_attrs = ()
    _model_id = _abi.MODEL_HBVADJ

    def _sources(self, T_total, B, ny, t_first, sta_row, dy_list, device):
        M = self.nmul
        srcs = []
        for i, name in enumerate(self.parameter_bounds.keys()):
            lo, hi = self.parameter_bounds[name]
            ps = ParamSource(slot=_abi.PARAM_SLOTS.index(name), lo=float(lo), hi=float(hi),
                             tensor_idx=0, sta_off=sta_row * B * ny + i * M, sta_bs=ny)
            if name in dy_list:
                ps.dyn_tensor_idx, ps.dyn_off = 0, t_first * B * ny + i * M
                ps.dyn_ts, ps.dyn_bs = B * ny, ny
                ps.drop = self._lane_drop_mask(B, device)
            srcs.append(ps)
        return srcs

    def forward(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor):
        """hbv_adj.py:227-330.  `graph=True`: HIP-graph replay of the call (graphed.py)."""
        if has_tangent(tuple(x_dict.values()), parameters):
            raise NotImplementedError("forward-mode AD (dual inputs) is not implemented for HbvAdj: "
                                      "Hbv, Hbv_1_1p and Hbv_2 support it; explicit directions go through "
                                      "HbvAdj.jvp_batch")
        if self.graph and x_dict['x_phy'].is_cuda:
            from hydrodl2_amd.graphed import graphed_forward
            return graphed_forward(self, x_dict, parameters)
        return self._forward_eager(x_dict, parameters)

    def jvp_batch(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor, tangents: dict,
                  max_directions: Optional[int] = None):
        """Implicit-function forward-mode derivatives of 'flow_sim' along many directions on one primal run:
        (outputs, tangents_out) = hydrodl2_amd.adj_jvp_batch(self, ...), see there."""
        from hydrodl2_amd.adj_jvp import adj_jvp_batch
        return adj_jvp_batch(self, x_dict, parameters, tangents, max_directions)

    def parameter_jacobian(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor, names=None,
                           max_directions: int = 64) -> dict:
        """Per-basin Jacobian of 'flow_sim' with respect to the static parameters:
        hydrodl2_amd.adj_parameter_jacobian(self, ...), see there."""
        from hydrodl2_amd.adj_jvp import adj_parameter_jacobian
        return adj_parameter_jacobian(self, x_dict, parameters, names, max_directions)

    def population_cost(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor, candidates: torch.Tensor,
                        target, names=None, weights=None, return_series: bool = False) -> dict:
        """The squared error of 'flow_sim' for many candidate static-parameter sets in one launch:
        hydrodl2_amd.adj_population_cost(self, ...), see there."""
        from hydrodl2_amd.adj_population import adj_population_cost
        return adj_population_cost(self, x_dict, parameters, candidates, target, names, weights, return_series)

    def population_stats(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor, candidates: torch.Tensor,
                         target, names=None, weights=None, transform: str = 'none', eps=None,
                         return_series: bool = False) -> dict:
        """The sums `hydrodl2_amd.population_score` turns into NSE, KGE and the like, per candidate:
        hydrodl2_amd.adj_population_stats(self, ...), see there."""
        from hydrodl2_amd.adj_population import adj_population_stats
        return adj_population_stats(self, x_dict, parameters, candidates, target, names, weights, transform, eps,
                                    return_series)

    def population_period_stats(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor,
                                candidates: torch.Tensor, target, periods=None, aux_target=None, aux_key=None,
                                aux_periods=None, names=None, weights=None, aux_weights=None, transform: str = 'none',
                                eps=None, return_series: bool = False) -> dict:
        """Scores against period means of 'flow_sim' and, optionally, of one storage ('SNOWPACK', 'MELTWATER', 'SM',
        'SUZ', 'SLZ'), per candidate: hydrodl2_amd.adj_population_period_stats(self, ...), see there."""
        from hydrodl2_amd.adj_population import adj_population_period_stats
        return adj_population_period_stats(self, x_dict, parameters, candidates, target, periods, aux_target, aux_key,
                                           aux_periods, names, weights, aux_weights, transform, eps, return_series)

    def population_search(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor, target, **kwargs):
        """Per-basin shrinking random search over the static row: hydrodl2_amd.adj_population_search(self, ...)."""
        from hydrodl2_amd.adj_population import adj_population_search
        return adj_population_search(self, x_dict, parameters, target, **kwargs)

    def _forward_eager(self, x_dict: dict[str, torch.Tensor], parameters: torch.Tensor,
                       state: Optional[torch.Tensor] = None):
        """hbv_adj.py:227-330.  `state` [5,B,nmul] (private: the tests' way to start from filled storages): the
        storages the first pass starts from -- the warm-up pass if there is one -- instead of zeros; differentiable."""
        x = x_dict['x_phy']
        T_total, B = x.shape[0], x.shape[1]
        M = self.nmul
        n = len(self.parameter_bounds)
        if not parameters.is_contiguous():
            parameters = parameters.contiguous()
        ny = parameters.shape[2]
        ch = (self.variables.index('prcp'), self.variables.index('tmean'),
              self.variables.index('pet'))
        wu = self.warm_up
        # The step configurations are functions of the shapes and the settings: built once and reused when no dy_drop
        # masks ride on them (their memo then also carries the persistent gradient buffer, grad_buffer='persistent')
        key = (T_total, B, ny, str(x.device), self._settings_key())
        hit = self._cfg_cache.get(key) if self.dy_drop <= 0 else None
        if hit is not None:
            cfg_w, cfg = hit
            self._advance_rng(B)                     # the draws _sources would have made (hbv_adj.py:182-189)
        else:
            base = dict(model=_abi.MODEL_HBVADJ, n_param=n, n_flux=1, B=B, M=M, raw_sigmoid=True,
                        channels=ch, nearzero=float(self.nearzero),
                        adj_gtol=float(self.newton_gtol), adj_max_iter=int(self.newton_max_iter),
                        adj_stop=2 if self.newton_solver == 'staged' else (1 if self.newton_stop == 'global' else 0),
                        persistent_grad=self.grad_buffer == 'persistent')
            cfg_w = None
            if wu > 0:  # hbv_adj.py:257-274: static parameters from row warm_up-1, differentiable
                cfg_w = StepConfig(T=wu, t0=0, want_flux=False, **base)
                cfg_w.params = self._sources(T_total, B, ny, 0, wu - 1, [], x.device)
            cfg = StepConfig(T=T_total - wu, t0=wu, **base)
            cfg.params = self._sources(T_total, B, ny, wu, T_total - 1, self.dynamic_params, x.device)
            if self.routing:
                off = (T_total - 1) * B * ny + n * M  # hbv_adj.py:151-153: last row only
                cfg.route = RouteSource(0, off, off + 1, ny,
                                        self.routing_parameter_bounds['rout_a'],
                                        self.routing_parameter_bounds['rout_b'])
            if self.dy_drop <= 0:
                if len(self._cfg_cache) > 8:
                    self._cfg_cache.clear()
                self._cfg_cache[key] = (cfg_w, cfg)
            else:
                # configurations with dy_drop masks are built per call; what is memoised on them (the library's size
                # answers, the persistent gradient buffer) is a function of the shapes and lives with the module
                if len(self._memo_cache) > 8:
                    self._memo_cache.clear()
                cfg.__dict__["_memo"] = self._memo_cache.setdefault(key, {})
        # state is None: zeros (hbv_adj.py:254)
        if cfg_w is not None:
            _, _, state = HbvAdjPath.apply(cfg_w, x, state, parameters)
        flux, routed, _ = HbvAdjPath.apply(cfg, x, state, parameters)
        q = routed if routed is not None else flux
        return {'flow_sim': q[0].unsqueeze(-1)}
