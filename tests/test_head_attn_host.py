"""The head's regional attention (use_interact_attention) without a GPU: the float64 restatement of
attn_cases pinned to the reference's fixture, the torch MultiHeadRegionalAttention and the whole CPU head
against them, the attention state dict through the checkpoint helpers, the constructors' refusals,
di_region_attn_check's contract (dummy pointers are never dereferenced), and the new ctypes struct
against the header."""
import ctypes

import pytest
import torch

import attn_cases as A
from deepinteract_amd import _lib
from deepinteract_amd.config import GeoTConfig
from test_capi import _declared_struct_fields

EINVAL, ERANGE = -1, -2
DEFAULT_SHA = "3484eeb2d7fb12c5cf74fcbffc442306cf0206b9e39b45e826eee85ee71bdff4"   # seeded_state_dict(0)
MHA_KEYS = [f"interact_module.MHA2D_{i}.{n}.weight" for i in (1, 2)
            for n in ("q_layer", "k_layer", "v_layer", "stretch_layer")]


def test_restatement_reproduces_the_fixture_blocks():
    """The fixture is the reference's fp32 output: ~1e-6 expected, 1e-5 required."""
    fx = A.fixture()
    for i in (1, 2):
        out, att = A.restate(fx[f"block{i}_in"][0], *A.block_weights(i))
        ref_out, ref_att = fx[f"block{i}_out"][0].double(), fx[f"block{i}_scores"].double()
        e_out = float((out - ref_out).abs().max() / ref_out.abs().max())
        e_att = float((att - ref_att).abs().max())
        print(f"block {i}: out rel {e_out:.2e}, attention weights abs {e_att:.2e}")
        assert e_out < 1e-5 and e_att < 1e-5


def test_restatement_border_rule_1x1():
    """A 1 x 1 image: v e^s / (e^s + 8)."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(128, 1, 1, generator=g, dtype=torch.float64)
    wq, wk = (torch.rand(16, 128, generator=g, dtype=torch.float64) - 0.5 for _ in range(2))
    wv = torch.randn(128, 128, generator=g, dtype=torch.float64)
    out, _ = A.restate(x, wq, wk, wv)
    s = A.scores64(x, wq, wk).repeat_interleave(32, 0)
    want = torch.einsum("oc,chw->ohw", wv, x) * s.exp() / (s.exp() + 8)
    assert torch.allclose(out, want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 3), (17, 33)])
def test_torch_module_matches_restatement(shape):
    from deepinteract_amd.head import MultiHeadRegionalAttention
    g = torch.Generator().manual_seed(2)
    m = MultiHeadRegionalAttention().double().eval()
    with torch.no_grad():
        for p in (m.q_layer.weight, m.k_layer.weight, m.v_layer.weight):
            p.copy_(torch.rand(p.shape, generator=g, dtype=torch.float64) * 0.5 - 0.25)
        x = torch.randn(1, 128, *shape, generator=g, dtype=torch.float64)
        out, att = m(x)
    want, want_att = A.restate(x[0], *(l.weight[:, :, 0, 0] for l in (m.q_layer, m.k_layer, m.v_layer)))
    assert out.shape == (1, 128, *shape) and att.shape == (4, 9, *shape)
    assert float((out[0] - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
    assert float((att - want_att).abs().max()) < 1e-13


def test_whole_cpu_head_matches_the_fixture():
    """The test that fails without the feature: the fixture's logits are those of the attention network."""
    fx = A.fixture()
    head = A.build_head()
    rec = {}
    for i in (1, 2):
        getattr(head, f"MHA2D_{i}").register_forward_hook(lambda m, a, o, i=i: rec.__setitem__(i, (a[0], o[0], o[1])))
    with torch.no_grad():
        logits = head(fx["input"])
    ref = fx["logits"]
    err = float((logits - ref).abs().max() / ref.abs().max())
    print(f"CPU head with attention vs the reference's: {err:.2e}")
    assert err < 1e-4
    for i in (1, 2):
        a, o, s = rec[i]
        scale = float(fx[f"block{i}_out"].abs().max())
        assert float((a - fx[f"block{i}_in"]).abs().max()) < 1e-4 * float(fx[f"block{i}_in"].abs().max())
        assert float((o - fx[f"block{i}_out"]).abs().max()) < 1e-4 * scale
        assert float((s - fx[f"block{i}_scores"]).abs().max()) < 1e-4
    # and the attention is not a no-op: the no-attention network on the same weights is far from it
    from deepinteract_amd.head import ResNet2DInputWithOptAttention
    plain = ResNet2DInputWithOptAttention(14, 256, 128, 2).eval()
    plain.load_state_dict({k: v for k, v in A.head_state_dict().items() if "MHA2D" not in k})
    with torch.no_grad():
        assert float((plain(fx["input"]) - ref).abs().max() / ref.abs().max()) > 1e-2


def test_fixture_weights_are_the_seeded_attention_state_dict():
    from deepinteract_amd.weights import state_dict_sha256
    assert A.fixture()["weights_sha256"] == state_dict_sha256(A.attention_state_dict())


# ---- state dicts --------------------------------------------------------------------------------
def test_default_state_dict_unchanged():
    from deepinteract_amd.weights import head_keys, seeded_state_dict, state_dict_sha256
    sd = seeded_state_dict(0)
    assert state_dict_sha256(sd) == DEFAULT_SHA
    assert not any("MHA2D" in k for k in sd)
    assert not any("MHA2D" in k for k, _, _ in head_keys())
    att = A.attention_state_dict()
    assert [k for k in att if k not in sd] == MHA_KEYS
    assert all(torch.equal(att[k], sd[k]) for k in sd)


def test_attention_checkpoint_round_trip(tmp_path):
    from deepinteract_amd.weights import (check_state_dict, infer_config, read_checkpoint, reference_init_state_dict,
                                          stretch_weight)
    sd = A.attention_state_dict()
    path = tmp_path / "attn.ckpt"
    torch.save({"state_dict": dict(sd), "hyper_parameters": {"use_interact_attention": True,
                                                             "num_interact_attention_heads": 4, "knn": 20}}, path)
    got, arch = read_checkpoint(str(path))
    assert arch["use_interact_attention"] is True and arch["num_interact_attention_heads"] == 4
    cfg = infer_config(got, **arch)
    assert cfg.use_interact_attention and cfg.num_interact_attention_heads == 4
    assert check_state_dict(got, cfg) == []
    # the flag follows the keys when the hyper-parameters are absent (a bare state dict)
    assert infer_config(got).use_interact_attention
    assert not infer_config({k: v for k, v in got.items() if "MHA2D" not in k}).use_interact_attention
    # a default build still refuses the attention keys, and an attention build misses them
    assert sorted(check_state_dict(got, GeoTConfig())) == sorted(f"unexpected {k}" for k in MHA_KEYS)
    from deepinteract_amd.weights import seeded_state_dict
    assert sorted(check_state_dict(seeded_state_dict(0), cfg)) == sorted(f"missing {k}" for k in MHA_KEYS)
    for k in MHA_KEYS:
        if "stretch" in k:
            assert torch.equal(sd[k], stretch_weight(3)) and sd[k].shape == (9, 1, 1, 3, 3)
    ri = reference_init_state_dict(0, GeoTConfig(use_interact_attention=True))
    assert [k for k in ri if "MHA2D" in k] == MHA_KEYS
    assert torch.equal(ri[MHA_KEYS[3]], stretch_weight(3))
    assert float(ri[MHA_KEYS[0]].abs().max()) <= 1 / 128 ** 0.5


def test_litgini_loads_an_attention_checkpoint(tmp_path):
    from deepinteract_amd.modules import LitGINI
    sd = A.attention_state_dict()
    path = tmp_path / "attn.ckpt"
    torch.save({"state_dict": dict(sd), "hyper_parameters": {"use_interact_attention": True}}, path)
    model = LitGINI.load_from_checkpoint(str(path))
    assert model.cfg.use_interact_attention and model.interact_module.use_attention
    assert torch.equal(model.interact_module.MHA2D_2.v_layer.weight, sd["interact_module.MHA2D_2.v_layer.weight"])
    plain = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {k: v for k, v in sd.items() if "MHA2D" not in k}}, plain)
    assert not LitGINI.load_from_checkpoint(str(plain)).interact_module.use_attention
    # a model built without the option refuses the checkpoint's extra keys
    with pytest.raises(RuntimeError, match="MHA2D"):
        LitGINI().load_reference_state_dict(sd)


def test_tampered_stretch_weight_is_refused():
    from deepinteract_amd.modules import LitGINI
    sd = dict(A.attention_state_dict())
    k = "interact_module.MHA2D_2.stretch_layer.weight"
    bad = sd[k].clone()
    bad[4, 0, 0, 1, 1], bad[4, 0, 0, 0, 1] = 0.0, 1.0   # the centre tap reads the pixel above
    sd[k] = bad
    with pytest.raises(ValueError, match="stretch"):
        LitGINI(use_interact_attention=True).load_reference_state_dict(sd)
    sd[k] = A.attention_state_dict()[k] * 0.5
    with pytest.raises(ValueError, match="stretch"):
        A.build_head().load_state_dict({k2[len("interact_module."):]: v for k2, v in sd.items()
                                        if k2.startswith("interact_module.")})


# ---- constructors -------------------------------------------------------------------------------
def test_constructor_refusals():
    from deepinteract_amd.head import MultiHeadRegionalAttention, ResNet2DInputWithOptAttention
    from deepinteract_amd.modules import LitGINI
    m = LitGINI(use_interact_attention=True, num_interact_attention_heads=4)
    assert m.cfg.use_interact_attention and hasattr(m.interact_module, "MHA2D_1")
    assert not LitGINI().cfg.use_interact_attention and not hasattr(LitGINI().interact_module, "MHA2D_1")
    assert LitGINI(num_interact_attention_heads=8).cfg.num_interact_attention_heads == 8   # unused without the option
    with pytest.raises(NotImplementedError):
        LitGINI(use_interact_attention=True, num_interact_attention_heads=8)
    with pytest.raises(ValueError, match="native"):
        LitGINI(use_interact_attention=True, head_dtype=torch.bfloat16, head_convs="hip", head_body="native")
    with pytest.raises(NotImplementedError):
        ResNet2DInputWithOptAttention(1, 256, 128, 2, use_attention=True, n_head=2)
    with pytest.raises(NotImplementedError):
        MultiHeadRegionalAttention(region_size=5)
    # every other mode constructs with the option
    for kw in (dict(), dict(head_dtype=torch.bfloat16), dict(head_dtype=torch.bfloat16, head_convs="hip"),
               dict(head_dtype=torch.bfloat16, head_convs="hip", head_batch=4), dict(fuse_head_prologue=True),
               dict(head_channels_last=True), dict(head_hip_ops=False)):
        assert LitGINI(use_interact_attention=True, **kw).interact_module.use_attention
    # GeoTConfig: the two fields come last, with defaults
    names = list(GeoTConfig.__dataclass_fields__)
    assert names[-2:] == ["use_interact_attention", "num_interact_attention_heads"]
    head = A.build_head()
    assert head.aops is None
    with pytest.raises(RuntimeError):   # body_batch is the HIP head's
        head.body_batch([torch.zeros(1, 128, 3, 3)])


def test_body_batch_native_refuses_attention():
    head = A.build_head()
    with pytest.raises(RuntimeError, match="native"):
        head.body_batch([torch.zeros(1, 128, 3, 3)], native=True)


# ---- C ABI --------------------------------------------------------------------------------------
def test_region_attn_struct_matches_header():
    assert [f for f, _ in _lib.DiRegionAttnArgs._fields_] == _declared_struct_fields("di_region_attn_args")
    assert ctypes.sizeof(_lib.DiRegionAttnArgs) == 6 * 8 + 3 * 4 + 4


def _args(h=17, w=33, **kw):
    P = 64 * 1024
    f = dict(x=P, wq=2 * P, wk=3 * P, scores=4 * P, v=5 * P, y=6 * P, h=h, w=w, in_elu=0)
    f.update(kw)
    return _lib.DiRegionAttnArgs(*(f[n] for n, _ in _lib.DiRegionAttnArgs._fields_))


def test_region_attn_check_contract():
    lib = _lib.load()
    chk = lambda dt, a: lib.di_region_attn_check(dt, ctypes.byref(a))   # noqa: E731
    for dt in (_lib.DI_F32, _lib.DI_BF16):
        assert chk(dt, _args()) == 0
        assert chk(dt, _args(1, 1)) == 0
        assert chk(dt, _args(4100, 4100)) == 0          # 128 h w > 2^31 elements: planes at 64-bit offsets
        assert chk(dt, _args(in_elu=1, y=64 * 1024)) == 0   # y may alias x
        assert lib.di_region_attn_check(dt, None) == EINVAL
        for bad in (dict(h=0), dict(w=0), dict(h=-3), dict(x=None), dict(wq=None), dict(wk=None), dict(scores=None),
                    dict(v=None), dict(y=None), dict(y=5 * 64 * 1024)):
            assert chk(dt, _args(**bad)) == EINVAL, bad
        for name in ("wq", "wk", "scores"):             # fp32 tensors: 4-B aligned
            assert chk(dt, _args(**{name: 64 * 1024 + 2})) == EINVAL
        for name in ("x", "v", "y"):                    # the element's own alignment, no more
            assert chk(dt, _args(**{name: 7 * 64 * 1024 + 1})) == EINVAL
            ok = 7 * 64 * 1024 + (2 if dt == _lib.DI_BF16 else 4)
            assert chk(dt, _args(**{name: ok})) == 0
        assert chk(_lib.DI_F32, _args(x=64 * 1024 + 2)) == EINVAL
        # 2^31 tiles of 256 pixels and more
        assert chk(dt, _args(2 ** 31 - 1, 256)) == 0
        assert chk(dt, _args(2 ** 31 - 1, 257)) == ERANGE
        assert chk(dt, _args(2 ** 31 - 1, 2 ** 31 - 1)) == ERANGE
    for dt in (2, 5, -1):
        assert chk(dt, _args()) == EINVAL


def test_region_calls_refuse_before_a_launch():
    """Each call checks the pointers it uses and ignores the other's; refusals come before any launch."""
    lib = _lib.load()
    dt = _lib.DI_BF16
    assert lib.di_region_scores(dt, ctypes.byref(_args(x=None)), None) == EINVAL
    assert lib.di_region_scores(dt, ctypes.byref(_args(scores=None)), None) == EINVAL
    assert lib.di_region_scores(dt, ctypes.byref(_args(h=0)), None) == EINVAL
    assert lib.di_region_scores(7, ctypes.byref(_args()), None) == EINVAL
    assert lib.di_region_mix(dt, ctypes.byref(_args(v=None)), None) == EINVAL
    assert lib.di_region_mix(dt, ctypes.byref(_args(y=5 * 64 * 1024)), None) == EINVAL
    assert lib.di_region_mix(dt, ctypes.byref(_args(scores=None)), None) == EINVAL
    assert lib.di_region_mix(dt, ctypes.byref(_args(2 ** 31 - 1, 2 ** 31 - 1)), None) == ERANGE
    assert lib.di_region_scores(dt, None, None) == EINVAL and lib.di_region_mix(dt, None, None) == EINVAL
    # the batch forms: the table's checks, then every item's
    from test_head_native_host import head_items
    items = head_items([(3, 5), (17, 33)])
    p = ctypes.c_void_p(64 * 1024)
    for fn in (lib.di_region_scores_batch, lib.di_region_mix_batch):
        assert fn(dt, None, items, p, 2, None) == EINVAL
        assert fn(dt, ctypes.byref(_args()), None, p, 2, None) == EINVAL
        assert fn(dt, ctypes.byref(_args()), items, None, 2, None) == EINVAL
        assert fn(dt, ctypes.byref(_args()), items, p, 0, None) == EINVAL
        assert fn(dt, ctypes.byref(_args()), head_items([(3, 5), (17, 33)], fill=False), p, 2, None) == EINVAL
        assert fn(9, ctypes.byref(_args()), items, p, 2, None) == EINVAL
    assert lib.di_region_scores_batch(dt, ctypes.byref(_args(wq=None)), items, p, 2, None) == EINVAL
    assert lib.di_region_mix_batch(dt, ctypes.byref(_args(y=5 * 64 * 1024)), items, p, 2, None) == EINVAL
