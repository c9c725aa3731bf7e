"""CPU tier: the host logic of hydrodl2_amd.sensitivity -- which columns a per-basin Jacobian runs through, the
compact one-hot directions, the pieces of max_directions, and which series a set of flux keys needs.  Tensor logic
only: nothing here calls the library."""
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.sensitivity import (direction_chunks, jacobian_columns, jvp_batch, one_hot_directions,
                                      parameter_jacobian, series_plan)

CPU = torch.device("cpu")


def _hbv(nmul=4, dyn=(), routing=True, cls="Hbv", mod="hbv"):
    return hydrodl2_amd.load_model(mod, cls)({"nmul": nmul, "routing": routing, "dynamic_params": {cls: list(dyn)}}, CPU)


def test_default_columns_are_every_static_parameter_and_the_routing_pair():
    m = _hbv(nmul=4)
    name, cols = jacobian_columns(m)
    assert name == "parameters"
    assert cols == list(range(12 * 4 + 2)) and len(cols) == m.learnable_param_count
    name, cols = jacobian_columns(_hbv(nmul=16))
    assert len(cols) == 194                                   # the headline model's raw static columns


def test_named_columns_follow_the_parameter_table_and_nmul():
    m = _hbv(nmul=3)
    assert jacobian_columns(m, ["parFC"])[1] == [3, 4, 5]                     # slot 1 of the table, nmul columns
    assert jacobian_columns(m, ["parCWH", "parBETA"])[1] == [33, 34, 35, 0, 1, 2]     # the order of `names`
    assert jacobian_columns(m, ["route_b", "route_a"])[1] == [37, 36]
    assert jacobian_columns(m, ["parK2", "route_a"])[1] == [12, 13, 14, 36]


def test_dynamic_parameters_shift_nothing_for_hbv_and_are_refused_by_name():
    m = _hbv(nmul=2, dyn=("parBETA", "parBETAET"))
    assert list(m.parameter_bounds)[-1] == "parBETAET"                        # 13 physical parameters
    name, cols = jacobian_columns(m)
    assert cols == list(range(2, 24)) + [26, 27]          # all but parBETA (0, 1) and parBETAET (24, 25); routing behind
    with pytest.raises(ValueError, match="dynamic parameter"):
        jacobian_columns(m, ["parFC", "parBETA"])
    with pytest.raises(ValueError, match="no static parameter"):
        jacobian_columns(m, ["parNOPE"])


def test_hbv2_columns_are_those_of_p_sta():
    m = _hbv(nmul=2, dyn=("parK0", "parBETA"), routing=True, cls="Hbv_2", mod="hbv_2")
    name, cols = jacobian_columns(m)
    assert name == "p_sta"
    assert cols == list(range(14 * 2 + 2)) and len(cols) == m.learnable_param_count2
    # parFC is the first static parameter of the table once parBETA is dynamic; parK1 the second (parK0 is dynamic too)
    assert jacobian_columns(m, ["parFC", "parK1", "route_a"])[1] == [0, 1, 2, 3, 28]
    with pytest.raises(ValueError, match="dynamic parameter"):
        jacobian_columns(m, ["parK0"])
    off = _hbv(nmul=2, routing=False, cls="Hbv_2", mod="hbv_2")
    assert jacobian_columns(off)[1] == list(range(32))
    with pytest.raises(ValueError, match="routing is off"):
        jacobian_columns(off, ["route_a"])


def test_one_hot_directions_are_compact_and_hit_every_basin():
    d = one_hot_directions([5, 0, 7], B=4, width=9)
    assert d.shape == (3, 4, 9) and d.dtype == torch.float32
    assert d.sum().item() == 3 * 4
    for c, col in enumerate([5, 0, 7]):
        assert (d[c, :, col] == 1).all() and d[c].sum().item() == 4
    assert one_hot_directions([], 4, 9).shape == (0, 4, 9)


def test_chunks_cover_the_columns_once():
    assert direction_chunks(194, 64) == [(0, 64), (64, 128), (128, 192), (192, 194)]
    assert direction_chunks(64, 64) == [(0, 64)]
    assert direction_chunks(3, 1) == [(0, 1), (1, 2), (2, 3)]
    assert direction_chunks(0, 8) == []
    with pytest.raises(ValueError):
        direction_chunks(5, 0)


def test_series_plan_asks_for_what_the_keys_need_only():
    F = _abi
    assert series_plan(["streamflow"], True, 11) == (1, 1, False)             # one series, one routed
    assert series_plan(["gwflow"], True, 11) == (0b1111, 4, False)            # routing runs over the leading series
    assert series_plan(["streamflow"], False, 12) == (1, 0, False)            # without routing it is Qsim itself
    assert series_plan(["BFI"], True, 11) == (0b1111, 4, True)
    assert series_plan(["BFI"], False, 12) == (0b1001, 0, True)
    assert series_plan(["SWE", "PET_hydro"], True, 11) == (1 << F.F_SWE, 0, False)
    assert series_plan(["capillary", "streamflow"], True, 12) == (1 | 1 << F.F_CAPILLARY, 1, False)
    with pytest.raises(KeyError):
        series_plan(["nonsense"], True, 11)


def test_refusals_need_no_device():
    m = _hbv()
    x = {"x_phy": torch.zeros(4, 2, 3)}
    p = torch.zeros(4, 2, m.learnable_param_count)
    with pytest.raises(ValueError, match="ac_all"):
        jvp_batch(m, x, p, {"ac_all": torch.zeros(1, 2)})
    with pytest.raises(ValueError, match="unknown tangent names"):
        jvp_batch(m, x, p, {"p_sta": torch.zeros(1, 2, 5)})
    with pytest.raises(ValueError, match="leading direction axis"):
        jvp_batch(m, x, p, {"parameters": torch.zeros(2, 2, 50), "x_phy": torch.zeros(3, 4, 2, 3)})
    m.graph = True
    with pytest.raises(ValueError, match="forward-mode AD"):
        jvp_batch(m, x, p, {"parameters": torch.zeros(1, 2, 50)})
    with pytest.raises(ValueError, match="forward-mode AD"):
        parameter_jacobian(m, x, p)
    for mod, cls in (("hbv_adj", "HbvAdj"), ("hbv_2_hourly", "Hbv_2_hourly")):
        other = hydrodl2_amd.load_model(mod, cls)(None, CPU)
        with pytest.raises(NotImplementedError, match="forward-mode AD"):
            jvp_batch(other, x, p, {"x_phy": torch.zeros(1, 4, 2, 3)})
        with pytest.raises(NotImplementedError, match="forward-mode AD"):
            parameter_jacobian(other, x, p)


def test_jacobian_pieces_share_one_primal_run(oracle_backend, monkeypatch):
    """parameter_jacobian differentiates ONE run of the module's forward, however many pieces of max_directions columns
    it takes: with cached states and dy_drop, the module (states, generator) ends where one plain call leaves it, and
    every piece is handed the records of that one run.  The primal runs on the CPU restatement of the library; the
    tangent step is replaced by a recorder (that restatement has no tangent kernels)."""
    from hydrodl2_amd import sensitivity

    def module():
        m = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": 2, "cache_states": True, "dy_drop": 0.5,
                                                  "dynamic_params": {"Hbv": ["parBETA"]}}, CPU)
        m.load_states(tuple(torch.full((B, 2), 3.0 + k) for k in range(5)))
        return m
    T, B = 5, 3
    ny = 12 * 2 + 2
    g = torch.Generator().manual_seed(3)
    x = {"x_phy": torch.rand((T, B, 3), generator=g) * 10.0}
    p = torch.randn((T, B, ny), generator=g)
    seen = []

    def fake(model, records, tangents, keys):
        seen.append((records, tangents["parameters"].clone()))
        D = tangents["parameters"].shape[0]
        return {k: torch.full((D, T, B, 1), float(len(seen))) for k in keys}
    monkeypatch.setattr(sensitivity, "_directional", fake)
    m = module()
    torch.manual_seed(11)
    J = parameter_jacobian(m, x, p, max_directions=10)
    after = torch.get_rng_state()
    cols = J["columns"]
    assert cols == list(range(2, 26))                 # 11 static parameters x 2 and the routing pair
    assert [t.shape[0] for _, t in seen] == [10, 10, 4]
    assert all(r is seen[0][0] for r, _ in seen) and len(seen[0][0]) == 1         # one run, one call of the path
    plain = module()
    torch.manual_seed(11)
    with torch.no_grad():
        plain(x, p)
    assert torch.equal(after, torch.get_rng_state())
    for a, b in zip(m.states, plain.states):
        assert torch.equal(a, b)
    assert not torch.equal(m.states[2], torch.full((B, 2), 5.0))                # ...and that call did move them
    assert J["streamflow"].shape == (T, B, 24)
    assert J["streamflow"][0, 0].tolist() == [1.0] * 10 + [2.0] * 10 + [3.0] * 4
    assert torch.equal(torch.cat([t for _, t in seen]), one_hot_directions(cols, B, ny))
    empty = parameter_jacobian(module(), x, p, names=[])
    assert empty["columns"] == [] and empty["streamflow"].shape == (T, B, 0)


def test_path_records_are_per_thread(oracle_backend):
    """ops.record_paths() sees the path calls of its own thread only."""
    import threading
    from hydrodl2_amd import ops
    m = _hbv(nmul=2)
    x = {"x_phy": torch.rand(4, 2, 3)}
    p = torch.randn(4, 2, 26)
    with ops.record_paths() as records:
        t = threading.Thread(target=lambda: m(x, p))
        t.start()
        t.join()
        assert records == []
        m(x, p)
    assert len(records) == 1 and records[0].cfg.T == 4
    m(x, p)
    assert len(records) == 1
