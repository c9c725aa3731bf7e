"""CPU tier: the public attribute surface of every model class, as the REFERENCE itself shows it, compared with this
package's class built from the same config.  SURVEY.md §8b lists the attributes callers read (hbv.py:43-105,172-180;
hbv_2.py:182-188).  What the reference shows -- attribute values, model discovery, what it refuses -- was read off it by
tests/golden/make_golden.py (`api` target) into tests/golden/reference_api.json; nothing of the reference travels."""
import json
import os

import pytest
import torch

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_api.json")

ATTRS = ["name", "initialize", "warm_up", "pred_cutoff", "warm_up_states", "dynamic_params", "dy_drop", "variables",
         "routing", "comprout", "nearzero", "nmul", "cache_states", "states", "state_names", "flux_names",
         "parameter_bounds", "routing_parameter_bounds", "phy_param_names", "routing_param_names",
         "learnable_param_count", "learnable_param_count1", "learnable_param_count2"]

CONFIGS = [
    ("hbv", "Hbv", None),
    ("hbv", "Hbv", {"nmul": 16, "warm_up": 30, "dy_drop": 0.2, "dynamic_params": {"Hbv": ["parBETA", "parBETAET"]}}),
    ("hbv", "Hbv", {"nmul": 2, "warm_up": 10, "warm_up_states": False, "routing": False, "nearzero": 1e-6,
                    "variables": ["tmean", "pet", "prcp"], "cache_states": True, "dynamic_params": {"Hbv": []}}),
    ("hbv_1_1p", "Hbv_1_1p", None),
    ("hbv_1_1p", "Hbv_1_1p", {"nmul": 4, "dynamic_params": {"Hbv_1_1p": ["parC", "parBETA"]}}),
    ("hbv_2", "Hbv_2", None),
    ("hbv_2", "Hbv_2", {"nmul": 4, "routing": True, "dynamic_params": {"Hbv_2": ["parBETA", "parK0", "parBETAET"]}}),
    ("hbv_2_hourly", "Hbv_2_hourly", None),
    ("hbv_2_hourly", "Hbv_2_hourly", {"nmul": 2, "routing": True, "dynamic_params": {"Hbv_2_hourly": ["parBETA", "parF0"]}}),
]


# what load_states is handed in test_load_states_rejects_what_the_reference_rejects (the record keeps them in this order)
BAD_STATES = [(torch.zeros(2, 1),) * 4, [torch.zeros(2, 1)] * 5, (1, 2, 3, 4, 5)]


@pytest.fixture(scope="module")
def reference():
    with open(RECORD) as f:
        return json.load(f)


def _plain(v):
    """A value as the record holds it (tensors as lists, through JSON)."""
    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        if isinstance(v, (set, frozenset, type({}.keys()))):     # compared as a set
            return sorted(conv(x) for x in v)
        if isinstance(v, (torch.device, torch.dtype)):
            return str(v)
        if torch.is_tensor(v):
            return v.tolist()
        return v
    return json.loads(json.dumps(conv(v)))


def _raises(fn):
    try:
        fn()
    except Exception as ex:  # noqa: BLE001
        return type(ex).__name__
    return None


@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=[f"{c[1]}-{i}" for i, c in enumerate(CONFIGS)])
def test_public_attributes_equal_the_references(i, reference):
    import warnings
    import hydrodl2_amd
    dev = torch.device("cpu")
    family, cls, cfg = CONFIGS[i]
    rec = reference["configs"][i]
    assert (rec["family"], rec["cls"], rec["config"]) == (family, cls, _plain(cfg))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        own = hydrodl2_amd.load_model(family, cls)(None if cfg is None else dict(cfg), dev)
    diffs = []
    for a, rv in rec["attrs"].items():
        assert hasattr(own, a), f"{cls}: attribute {a!r} of the reference is missing"
        ov = _plain(getattr(own, a))
        if rv != ov:
            diffs.append(f"{a}: reference {rv!r} != {ov!r}")
    assert not diffs, f"{cls} {cfg}: " + "; ".join(diffs)
    # dict ORDER matters to callers that zip names with columns
    for a in ("parameter_bounds", "flux_names", "state_names"):
        assert rec["order"][a] == list(getattr(own, a)), a


def test_model_discovery_equals_the_references(reference):
    """`available_models()` (api/methods.py:78-139): same families and class files, minus what cannot be imported upstream
    (hbv_adj needs an encrypted dependency there; here it loads)."""
    import hydrodl2_amd
    ref, own = reference["available_models"], hydrodl2_amd.available_models()
    assert set(ref) <= set(own), (ref, own)
    for fam, names in ref.items():
        assert set(names) <= set(own[fam]), (fam, names, own[fam])
    # an unknown name: the reference means to raise ImportError("Model '...' not found.") (api/methods.py:116-117) but only
    # catches ImportError around the file load, so the missing FILE surfaces as FileNotFoundError; this package raises the
    # ImportError the reference words.  Pinned here so that the difference is a recorded one
    assert reference["load_unknown_family_raises"] == "FileNotFoundError"
    with pytest.raises(ImportError, match="not found"):
        hydrodl2_amd.load_model("no_such_family")
    # an unknown class in a known file: both fall back to the first class of the module (api/methods.py:123-137)
    assert reference["load_unknown_class_returns"] == hydrodl2_amd.load_model("hbv", "Nope").__name__ == "Hbv"


@pytest.mark.parametrize("i", range(len(BAD_STATES)), ids=[f"bad{i}" for i in range(len(BAD_STATES))])
def test_load_states_rejects_what_the_reference_rejects(i, reference):
    import hydrodl2_amd
    dev = torch.device("cpu")
    assert reference["load_states_raises"][i] == "ValueError"
    m = hydrodl2_amd.load_model("hbv", "Hbv")(None, dev)
    with pytest.raises(ValueError):
        m.load_states(BAD_STATES[i])


def test_multi_timescale_wrapper_has_the_references_surface(reference):
    """Hbv_2_mts(low_freq_config, high_freq_config, device) (hbv_2_mts.py:31-75): every public data attribute the
    reference's instance carries exists here with the same value; sub-models are the same classes in the same roles.
    (The reference indexes high_freq_config for its chunk sizes: a config without them is a TypeError there and here.)"""
    import warnings
    import hydrodl2_amd
    from . import golden_mts
    dev = torch.device("cpu")
    rec = reference["mts"]
    low, high = golden_mts.configs("mts_chunked")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        own = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")(dict(low), dict(high), dev)
        assert rec["no_config_raises"] == "TypeError"
        with pytest.raises(TypeError):
            hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")(None, None, dev)
    diffs = []
    for a, rv in rec["attrs"].items():
        assert hasattr(own, a), f"Hbv_2_mts: attribute {a!r} of the reference is missing"
        ov = getattr(own, a)
        if "module" in rv:
            if rv["module"] != type(ov).__name__:
                diffs.append(f"{a}: {rv['module']} != {type(ov).__name__}")
        elif rv["value"] != _plain(ov):
            diffs.append(f"{a}: reference {rv['value']!r} != {_plain(ov)!r}")
    assert not diffs, diffs
    assert rec["sub"]["low_freq_model"]["initialize"] is True and own.low_freq_model.initialize is True
    for sub in ("low_freq_model", "high_freq_model"):
        o = getattr(own, sub)
        for a, rv in rec["sub"][sub].items():
            assert rv == _plain(getattr(o, a)), (sub, a)
