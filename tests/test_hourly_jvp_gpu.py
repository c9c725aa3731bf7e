"""GPU tier: Hbv_2_hourly.jvp_batch (hydrodl2_amd.hourly_jvp_batch) on the eight hourly golden cases against float64
forward AD of oracle/hbv_restate64.py's run_hourly: 'Qs' and 'streamflow' at TAN_RTOL + TAN_ATOL_REL x max|float64
tangent of the key| under hourly_sets.admit.  Around it: the primal outputs and the module's state after the call are
those of one plain call, max_directions splits the tangent calls only, the tangent is linear in the direction, and
what the path cannot differentiate is refused."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from . import golden_cases as gc
from . import hourly_jvp_util as hu

pytestmark = pytest.mark.gpu

DEV = "cuda"
A, Bc = 0.75, -1.5          # the linear combination of (c)
_WANT = {}


def _model(name, **over):
    import hydrodl2_amd
    cfg = dict(gc.CASES[name]["config"])
    cfg.update(over)
    return hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")(cfg, torch.device(DEV))


def _args(name, inp):
    t = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in inp.items()}
    x_dict = {k: t[k] for k in ("x_phy", "ac_all", "elev_all", "outlet_topo", "areas", "muwts") if k in t}
    return x_dict, (t["p_dyn"], t["p_sta"], t["p_distr"]), t


def _prepare(name, model, inp):
    """What helpers.run_case does before the call: carried-in storages, the generator's seed."""
    spec = gc.CASES[name]
    if "states0" in inp:
        model.load_states(tuple(torch.from_numpy(s.copy()).to(DEV) for s in inp["states0"]))
    torch.manual_seed(spec.get("torch_seed", 0))     # (a case without dy_drop names no seed: any, the same for both)


def _tangents(dirs_list):
    names = {"states0": "states"}
    return {names.get(k, k): torch.from_numpy(np.stack([d[k] for d in dirs_list])).to(DEV) for k in dirs_list[0]}


def _jvp(name, inp, dirs_list, **kw):
    model = _model(name)
    _prepare(name, model, inp)
    x_dict, params, _ = _args(name, inp)
    out, tan = model.jvp_batch(x_dict, params, _tangents(dirs_list), **kw)
    torch.cuda.synchronize()
    return model, out, {k: v.cpu().numpy() for k, v in tan.items()}


def _module_state(model):
    st = model.get_states()
    return dict(series=None if st is None else [s.cpu().numpy() for s in st],
                states=None if not model.states else [s.cpu().numpy() for s in model.states],
                buffer=[q.cpu().numpy() for q in model._qs_buffer], rng=torch.get_rng_state().numpy())


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a, b)


def _want(name, inp, dirs):
    if name not in _WANT:
        _WANT[name] = hu.module_forward_ad(name, inp, dirs)
    return _WANT[name]


@pytest.mark.parametrize("name", hu.HOURLY_CASES)
def test_tangents_against_float64_on_one_plain_primal(name, hip_backend):
    inp = gc.build_inputs(name)
    u, v = hu.module_directions(inp, 41), hu.module_directions(inp, 42)
    comb = {k: (A * u[k] + Bc * v[k]).astype(np.float32) for k in u}
    model, out, tan = _jvp(name, inp, [u, v, comb])
    after = _module_state(model)

    # (a) against float64 forward AD, direction u
    want = _want(name, inp, u)
    assert set(tan) == {"Qs", "streamflow"}
    top = max(float(np.abs(w).max()) for w in want.values())
    f32 = {}

    def alt(k):
        def f():
            if not f32:
                f32.update(hu.module_forward_ad(name, inp, u, torch.float32))
            return f32[k][None]
        return f
    for k in ("Qs", "streamflow"):
        assert tan[k].shape == (3,) + want[k].shape, (k, tan[k].shape, want[k].shape)
        hu.compare(f"hourly-jvp:{name}:{k}", tan[k][0][None], want[k][None], alt(k), top=top)
    assert top > 0

    # (b) the primal outputs and the module afterwards are one plain call's
    plain = _model(name)
    _prepare(name, plain, inp)
    x_dict, params, _ = _args(name, inp)
    with torch.no_grad():
        ref = plain(x_dict, params)
    assert set(out) == set(ref)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    want_state = _module_state(plain)
    for k in want_state:
        assert _same(after[k], want_state[k]), k

    # (c) JVP(a u + b v) == a JVP(u) + b JVP(v), at the default tolerance (of the combination's own size)
    for k in ("Qs", "streamflow"):
        lin = A * tan[k][0].astype(np.float64) + Bc * tan[k][1].astype(np.float64)
        tol = hu.tan_tol(max(float(np.abs(lin).max()), 1e-300))(lin[None])[0]
        err = np.abs(tan[k][2] - lin)
        print(f"hourly-jvp-linear:{name}:{k}: worst error / tolerance {float((err / tol).max()):.3g}")
        assert (err <= tol).all(), (name, k, float((err / tol).max()))


@pytest.mark.parametrize("name", ["hourly_routing_drop", "hourly_wet_routing", "hourly_wet_muwts"])
def test_max_directions_splits_the_tangent_calls_only(name, hip_backend):
    inp = gc.build_inputs(name)
    five = [hu.module_directions(inp, 41 + d) for d in range(5)]
    _, out5, tan5 = _jvp(name, inp, five)
    _, out2, tan2 = _jvp(name, inp, five, max_directions=2)
    for k in tan5:
        assert tan5[k].shape[0] == 5
        assert np.array_equal(tan5[k], tan2[k]), k
        assert torch.equal(out5[k], out2[k]), k
    _, _, only = _jvp(name, inp, five, keys=("streamflow",))
    assert set(only) == {"streamflow"} and np.array_equal(only["streamflow"], tan5["streamflow"])


def test_refusals(hip_backend):
    name = "hourly_dyn3"
    inp = gc.build_inputs(name)
    x_dict, params, t = _args(name, inp)
    one = {"p_sta": torch.ones((2,) + tuple(t["p_sta"].shape), device=DEV)}
    model = _model(name)
    for fixed in ("ac_all", "elev_all", "outlet_topo", "areas"):
        with pytest.raises(ValueError, match=fixed):
            model.jvp_batch(x_dict, params, dict(one, **{fixed: torch.ones((2,) + tuple(t[fixed].shape), device=DEV)}))
    with pytest.raises(ValueError, match="unknown tangent names"):
        model.jvp_batch(x_dict, params, dict(one, parameters=one["p_sta"]))
    with pytest.raises(ValueError, match="leading direction axis"):
        model.jvp_batch(x_dict, params, dict(one, p_distr=torch.ones((3,) + tuple(t["p_distr"].shape), device=DEV)))
    with pytest.raises(ValueError, match="full form"):
        model.jvp_batch(x_dict, params, {"p_dyn": torch.ones((2,) + tuple(t["p_dyn"].shape[1:]), device=DEV)})
    with pytest.raises(ValueError, match="max_directions"):
        model.jvp_batch(x_dict, params, one, max_directions=0)
    with pytest.raises(KeyError):
        model.jvp_batch(x_dict, params, one, keys=("BFI",))
    with pytest.raises(ValueError, match="graph=True"):
        _model(name, graph=True).jvp_batch(x_dict, params, one)
    init = _model(name)
    init.initialize = True
    with pytest.raises(ValueError, match="initialize"):
        init.jvp_batch(x_dict, params, one)
    # the dual-tensor path and the generic entry points keep refusing the model
    import hydrodl2_amd
    with fwAD.dual_level():
        dual = fwAD.make_dual(t["p_sta"], torch.ones_like(t["p_sta"]))
        with pytest.raises(NotImplementedError, match="forward-mode AD"):
            model(x_dict, (t["p_dyn"], dual, t["p_distr"]))
    with pytest.raises(NotImplementedError, match="forward-mode AD"):
        hydrodl2_amd.jvp_batch(model, x_dict, params, one)
    assert hydrodl2_amd.hourly_jvp_batch(model, x_dict, params, one)[1]["Qs"].shape[0] == 2
