"""Which forwards take the z0 path (engine.uses_z_init / GeoTEngine.z_init): host-side selection
logic only, on stub engine and batch objects (no GPU, no library call)."""
import types

import pytest

from deepinteract_amd import engine
from deepinteract_amd.engine import uses_z_init


def _eng(z_init=True, dtype="bf16", fuse=True, fold=False, layers=2):
    return types.SimpleNamespace(z_init=z_init, dtype=dtype, fuse_embed_init=fuse, fold_attn=fold,
                                 packed=types.SimpleNamespace(num_layers=layers))


def _gb(geo_ref=True):
    return types.SimpleNamespace(geo_ref=geo_ref)


def test_default_configuration_takes_the_z_path():
    assert uses_z_init(_eng(), _gb()) is True
    assert uses_z_init(_eng(layers=4), _gb()) is True


@pytest.mark.parametrize("eng_kw, geo_ref", [
    ({"dtype": "f32"}, True),   # the fp32 kernels keep F0
    ({}, False),                # the general path also gathers Fn rows computed from F0
    ({"fuse": False}, True),    # di_init_edge / di_init_edge_resident write F0
    ({"fold": True}, True),     # no di_edge_layer_attn form
    ({"layers": 1}, True),      # layer 0 is the final layer
    ({"z_init": False}, True),
])
def test_each_condition_alone_keeps_the_f_path(eng_kw, geo_ref):
    assert uses_z_init(_eng(**eng_kw), _gb(geo_ref)) is False


class _StubLib:
    """What GeoTEngine.__init__ asks of the library: layouts and blob sizes."""

    def di_blob_layout(self, kind, dt):
        return 32 if dt == 1 and kind in (1, 2, 3) else 16


@pytest.mark.parametrize("value, want", [(None, True), ("1", True), ("0", False)])
def test_environment_override_is_read_at_construction(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("DI_INIT_Z", raising=False)
    else:
        monkeypatch.setenv("DI_INIT_Z", value)
    monkeypatch.setattr(engine, "gpu_device", lambda d: d)
    monkeypatch.setattr(engine._lib, "load", lambda: _StubLib())
    monkeypatch.setattr(engine, "PackedGeoT", lambda *a, **k: types.SimpleNamespace(num_layers=2))
    monkeypatch.setattr(engine.GeoTEngine, "_check_blob_sizes", lambda self: None)
    e = engine.GeoTEngine({}, "bf16", device="cpu")
    assert e.z_init is want
    assert uses_z_init(e, _gb()) is want
    # read once: a later change of the environment does not move an existing engine
    monkeypatch.setenv("DI_INIT_Z", "0" if want else "1")
    assert e.z_init is want
