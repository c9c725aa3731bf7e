"""HBV 2.0 multi-timescale on the MI355X-native time-stepper.

Counterpart of `hydrodl2.load_model('hbv_2_mts', 'Hbv_2_mts')`
(src/hydrodl2/models/hbv/hbv_2_mts.py:10-377): a daily `Hbv_2` run warms the five storages up
(no gradient: the hand-off is detached, hbv_2.py:388), the hourly model continues from them with
the daily model's static parameters plus its own (parF0, parFMIN, parALPHA, dynamic ones), and
gage routing runs over the concatenated unit runoff in temporal chunks with `train_warmup`
overlap.  Spatial chunks stream host tensors to the device one block of units at a time.

This module is orchestration only: every number comes from `hbvx_forward` / `hbvx_backward` /
`hbvx_gage_route_*` through the two sub-models.

Differences from the reference, all on lines that cannot run there:
  * `hbv_2_mts.py:246` calls `high_freq_model.unpack_parameters` and `:338`
    `_descale_rout_parameters`; neither exists (the methods are `_unpack_parameters`,
    `_descale_route_parameters`).  The evident intent is implemented.
  * the parameter hand-off (`param_transfer`, :292-341) is positional: hourly static parameter
    i takes column i of [daily static | hourly-only static]; kept as is, with a ValueError
    instead of an IndexError when the two lists do not line up.
"""
from typing import Any, Optional

import torch
from tqdm import tqdm

from hydrodl2_amd import _abi
from hydrodl2_amd.models.hbv.hbv_2 import Hbv_2
from hydrodl2_amd.models.hbv.hbv_2_hourly import Hbv_2_hourly
from hydrodl2_amd.ops import ParamSource, has_tangent


class Hbv_2_mts(torch.nn.Module):
    """HBV 2.0, multi timescale, distributed UH."""

    # chunking keys of the hourly config (hbv_2_mts.py:65-76) -> attribute of the same name
    _CHUNK_KEYS = ('train_spatial_chunk_size', 'simulate_spatial_chunk_size',
                   'simulate_temporal_chunk_size', 'train_warmup')

    def __init__(self, low_freq_config: Optional[dict[str, Any]] = None,
                 high_freq_config: Optional[dict[str, Any]] = None,
                 device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.device = torch.device('cpu') if device is None else device
        self.dtype = torch.float32
        daily, hourly = Hbv_2(low_freq_config, device=device), Hbv_2_hourly(high_freq_config, device=device)
        if daily.nmul != hourly.nmul:
            raise ValueError("low- and high-frequency models must share nmul "
                             "(the static parameters are concatenated, hbv_2_mts.py:326-329)")
        daily.initialize = True            # the daily run only warms the storages up
        self.low_freq_model, self.high_freq_model = daily, hourly
        self.state_transfer_model = torch.nn.ModuleDict(
            {name: torch.nn.Identity() for name in hourly.state_names})
        for key in self._CHUNK_KEYS:
            setattr(self, key, high_freq_config[key])
        self._state_cache = [None, None]   # [daily series, hourly series]
        self.states = (None, None)
        self.load_from_cache = self.use_from_cache = False
        self.set_mode(False)

    # -- state API (hbv_2_mts.py:78-98) -------------------------------------------------------
    def get_states(self):
        """(daily state series, hourly state series).  The hourly series is the one `_forward`
        cached: the hourly sub-model is driven through `_PBM`, which does not fill its own cache
        (upstream returns None there, so `load_states(get_states())` could not round-trip)."""
        hourly = self.high_freq_model.get_states()
        if hourly is None:
            hourly = self._state_cache[1]
        return (self.low_freq_model.get_states(), hourly)

    def load_states(self, state_tuple) -> None:
        if not (isinstance(state_tuple, tuple) and len(state_tuple) == 2):
            raise ValueError("`states` must be a tuple of two tuples of tensors.")

        def last_step(series):
            return tuple(s[-1].detach().to(self.device, dtype=self.dtype) for s in series)

        self._state_cache = (last_step(state_tuple[0]), last_step(state_tuple[1]))
        if self.load_from_cache:
            self.low_freq_model.load_states(state_tuple[0])

    def set_mode(self, is_simulate: bool):
        """Training blocks vs simulation blocks of units (hbv_2_mts.py:283-290)."""
        self.simulate_mode = bool(is_simulate)
        self.spatial_chunk_size = (self.simulate_spatial_chunk_size if self.simulate_mode
                                   else self.train_spatial_chunk_size)

    # -- hand-offs ----------------------------------------------------------------------------
    def state_transfer(self, states):
        """hbv_2_mts.py:343-349 (identity per storage)."""
        if states is None:
            raise ValueError("the low-frequency model kept no states: set cache_states=True in "
                             "low_freq_config (hbv_2.py:387-388)")
        names = self.high_freq_model.state_names
        return [self.state_transfer_model[k](s) for k, s in zip(names, states)]

    def param_transfer(self, low_freq_parameters, high_freq_parameters, T: int, ngrid: int, device):
        """Where the hourly model's 19 parameters come from (hbv_2_mts.py:292-341).

        Returns (sources, tensors): tensors = (hourly dynamic, hourly static, daily static)."""
        hi, lo = self.high_freq_model, self.low_freq_model
        M = hi.nmul
        p_dyn = high_freq_parameters[0].contiguous()
        p_sta = high_freq_parameters[1].contiguous()
        lo_sta = low_freq_parameters[1].contiguous()
        wd, ws, wl = p_dyn.shape[-1], p_sta.shape[-1], lo_sta.shape[-1]
        dy = list(hi.dynamic_params)
        if wd != len(dy) * M:
            raise ValueError(f"dynamic parameters have {wd} columns, need {len(dy) * M}")
        static_names = [n for n in hi.phy_param_names if n not in dy]
        warm_static = [n for n in lo.phy_param_names if n not in lo.dynamic_params]
        var_indexes = [i for i, n in enumerate(static_names) if n not in warm_static]
        if len(warm_static) + len(var_indexes) < len(static_names):
            raise ValueError("daily static + hourly-only static parameters do not cover the hourly "
                             "static list (hbv_2_mts.py:326-331)")
        if wl < len(warm_static) * M:
            raise ValueError(f"daily static parameters have {wl} columns, need {len(warm_static) * M}")
        srcs = []
        for name in hi.parameter_bounds:
            b0, b1 = hi.parameter_bounds[name]
            slot = _abi.PARAM_SLOTS.index(name)
            if name in dy:
                i = dy.index(name)
                srcs.append(ParamSource(slot=slot, lo=float(b0), hi=float(b1), tensor_idx=0,
                                        sta_off=(T - 1) * ngrid * wd + i * M, sta_bs=wd,
                                        dyn_tensor_idx=0, dyn_off=i * M, dyn_ts=ngrid * wd,
                                        dyn_bs=wd, drop=hi._draw_drop_mask(ngrid, device)))
                continue
            i = static_names.index(name)
            if i < len(warm_static):       # column i of the daily static block
                srcs.append(ParamSource(slot=slot, lo=float(b0), hi=float(b1), tensor_idx=2,
                                        sta_off=i * M, sta_bs=wl))
            else:                          # hourly-only static parameter
                j = var_indexes[i - len(warm_static)]
                srcs.append(ParamSource(slot=slot, lo=float(b0), hi=float(b1), tensor_idx=1,
                                        sta_off=j * M, sta_bs=ws))
        return srcs, (p_dyn, p_sta, lo_sta)

    # -- one block of units -------------------------------------------------------------------
    def _forward(self, x_dict, parameters):
        """hbv_2_mts.py:100-174."""
        low_freq_parameters, high_freq_parameters = parameters
        hi, lo = self.high_freq_model, self.low_freq_model
        if self.use_from_cache and (self._state_cache[1] is not None):
            states = self.states[1]
        else:
            lo.states = None
            with torch.no_grad():          # the hand-off is detached (hbv_2.py:388)
                lo({'x_phy': x_dict['x_phy_low_freq'], 'ac_all': x_dict['ac_all'],
                    'elev_all': x_dict['elev_all'], 'muwts': x_dict.get('muwts', None)},
                   low_freq_parameters)
            self._state_cache[0] = lo.states
            states = self.state_transfer(lo.states)

        x = x_dict['x_phy_high_freq']
        T, ngrid = x.shape[0], x.shape[1]
        srcs, tensors = self.param_transfer(low_freq_parameters, high_freq_parameters, T, ngrid,
                                            x.device)
        p_route = None
        if hi.routing:
            n_sta = len(hi.parameter_bounds) - len(hi.dynamic_params)
            p_route = tensors[1][:, n_sta * hi.nmul: n_sta * hi.nmul + 2]
        state_in = hi._stack_states(tuple(states), ngrid, x.device)
        predictions, hif_states = hi._PBM(x, x_dict['ac_all'], x_dict['elev_all'], state_in, srcs,
                                          tensors, x_dict['outlet_topo'], x_dict['areas'],
                                          high_freq_parameters[2], p_route)
        self._state_cache[1] = tuple(s.detach() for s in hif_states)
        if self.load_from_cache:
            self.states = (self._state_cache[0], tuple(s[-1] for s in hif_states))
        return predictions

    # -- chunked driver -----------------------------------------------------------------------
    @staticmethod
    def _unit_blocks(n_units: int, size: int):
        """Consecutive [lo, hi) blocks of units."""
        for lo in range(0, n_units, size):
            yield lo, min(lo + size, n_units)

    @staticmethod
    def _routing_windows(n_steps: int, warmup: int, size: int):
        """(first row read, one past the last row, rows to drop) per temporal routing window:
        every window re-reads `warmup` rows of history; only the first keeps them in its output
        (hbv_2_mts.py:254-278)."""
        for start in range(warmup, n_steps, size):
            yield start - warmup, min(start + size, n_steps), (0 if start == warmup else warmup)

    def _block_inputs(self, x_dict, parameters, lo, hi, pair_unit):
        """Unit block [lo, hi) of every input, on the compute device.  `pair_unit[k]` = unit of
        gage-unit pair k, so the block's pair parameters are the rows with lo <= unit < hi."""
        dev = self.device
        (day_dyn, day_sta), (hr_dyn, hr_sta, hr_pair) = parameters[0][:2], parameters[1][:3]
        xs = {k: x_dict[k][:, lo:hi].to(dev) for k in ('x_phy_low_freq', 'x_phy_high_freq', 'outlet_topo')}
        xs.update({k: x_dict[k][lo:hi].to(dev) for k in ('ac_all', 'elev_all', 'areas')})
        in_block = (pair_unit >= lo) & (pair_unit < hi)
        ps = ([day_dyn[:, lo:hi].to(dev), day_sta[lo:hi].to(dev)],
              [hr_dyn[:, lo:hi].to(dev), hr_sta[lo:hi].to(dev), hr_pair[in_block].to(dev)])
        return xs, ps

    def forward(self, x_dict, parameters):
        """Whole-domain run (hbv_2_mts.py:176-281).  Small training batches go through `_forward`
        in one piece.  Otherwise the unit runoff is produced block by block (inputs may live on
        the host; a block is moved to the device when its turn comes) without gage routing, and
        the gage routing then runs over the assembled runoff in temporal windows."""
        if has_tangent(tuple(x_dict.values()), parameters):
            raise NotImplementedError("forward-mode AD (dual inputs) is not implemented for Hbv_2_mts: "
                                      "Hbv, Hbv_1_1p and Hbv_2 support it")
        hourly = self.high_freq_model
        n_units = x_dict['areas'].shape[0]
        hourly.use_distr_routing = False
        if not self.simulate_mode and n_units <= self.spatial_chunk_size:
            return self._forward(x_dict, parameters)

        pair_unit = (x_dict['outlet_topo'] == 1).nonzero(as_tuple=False)[:, 1]   # once, not per block
        blocks = list(self._unit_blocks(n_units, self.spatial_chunk_size))
        per_block = [self._forward(*self._block_inputs(x_dict, parameters, lo, hi, pair_unit))
                     for lo, hi in tqdm(blocks, desc="Spatial runoff chunks")]
        predictions = self.concat_spatial_chunks(per_block)

        runoff = predictions['Qs']
        topo, areas = x_dict['outlet_topo'].to(self.device), x_dict['areas'].to(self.device)
        pair_params = parameters[1][2].to(self.device)
        windows = list(self._routing_windows(runoff.shape[0], self.train_warmup,
                                             self.simulate_temporal_chunk_size))
        pieces = []
        for first, stop, drop in tqdm(windows, desc="Temporal routing chunks"):
            q = hourly.distr_routing(runoff[first:stop], pair_params, topo, areas)
            pieces.append({'Qs_rout': q[drop:]})
        predictions['streamflow'] = self.concat_temporal_chunks(pieces)['Qs_rout']
        return predictions

    @staticmethod
    def concat_spatial_chunks(pred_list):
        """Join per-block outputs on the unit axis: [T, units, 1] series on dim 1, per-unit
        vectors on dim 0 (hbv_2_mts.py:351-364)."""
        first = pred_list[0]
        return {k: torch.cat([p[k] for p in pred_list], dim=(1 if first[k].ndim == 3 else 0)) for k in first}

    @staticmethod
    def concat_temporal_chunks(pred_list):
        """Join per-window outputs on the time axis; anything that is not a [T, ., 1] series is
        taken from the first window (hbv_2_mts.py:366-377)."""
        first = pred_list[0]
        return {k: (torch.cat([p[k] for p in pred_list], dim=0) if first[k].ndim == 3 else first[k])
                for k in first}
