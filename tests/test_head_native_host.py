"""The native head body without a GPU: di_head_body_batch_check on a well-formed plan of the model's
shape (56 + 6 blocks) and every refusal the header lists, di_head_body_batch / di_head_logits_batch
refusing before a launch (dummy pointers are never dereferenced), the new ctypes structs against the
header, the plan head.HeadBodyPlan builds from a module, and LitGINI(head_body=...)'s validation."""
import ctypes

import pytest
import torch

from deepinteract_amd import _lib
from test_capi import _declared_arg_counts, _declared_struct_fields

EINVAL, ERANGE = -1, -2
P = 64 * 1024                      # dummy non-NULL, 16-B aligned pointers: P, 2P, ...
SHAPES = [(48, 40), (1, 1), (17, 9), (3, 5), (70, 33)]
DILATIONS = [(1, 2, 4, 8)[i % 4] for i in range(56)], [1, 2, 4, 8, 1, 1]


def head_items(shapes, fill=True):
    items = (_lib.DiHeadItem * len(shapes))()
    for it, (h, w) in zip(items, shapes):
        it.h, it.w = h, w
    if fill:   # (the helper lays out at most DI_BATCH_MAX items; a longer table is refused for its count)
        px, nb = ctypes.c_int64(), ctypes.c_int64()
        assert _lib.load().di_head_batch_layout(items, min(len(shapes), _lib.DI_BATCH_MAX), ctypes.byref(px),
                                                ctypes.byref(nb)) == 0
    return items


class Plan:
    """Two nets as the model has them: norms on the first only, in_elu on the second; an arena of six
    different dummy buffers. Holds the ctypes arrays alive."""

    def __init__(self, shapes=SHAPES):
        self.blocks = []
        for n, dils in enumerate(DILATIONS):
            arr = (_lib.DiHeadBlock * len(dils))()
            for blk, d in zip(arr, dils):
                for name, _ in _lib.DiHeadBlock._fields_[:16]:
                    setattr(blk, name, P)
                if n == 1:
                    for i in (1, 2, 3):
                        setattr(blk, f"gamma{i}", None), setattr(blk, f"beta{i}", None)
                blk.eps, blk.dilation = 1e-6, d
            self.blocks.append(arr)
        self.nets = (_lib.DiHeadNet * 2)(_lib.DiHeadNet(P, P, self.blocks[0], 56, 0),
                                         _lib.DiHeadNet(P, P, self.blocks[1], 6, 1))
        self.items = head_items(shapes)
        self.arena = _lib.DiHeadArena(1 * P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P, ctypes.addressof(self.items), 7 * P,
                                      len(shapes))

    def check(self, dt=_lib.DI_BF16, nets="own", num_nets=2, arena="own"):
        return _lib.load().di_head_body_batch_check(dt, self.nets if nets == "own" else nets, num_nets,
                                                    ctypes.byref(self.arena) if arena == "own" else arena)


def test_well_formed_plan_passes():
    p = Plan()
    assert [b.dilation for b in p.blocks[0]] == [1, 2, 4, 8] * 14
    assert [b.dilation for b in p.blocks[1]] == [1, 2, 4, 8, 1, 1]
    assert p.check() == 0
    assert Plan([(1, 1)]).check() == 0 and Plan([(1000, 1000)] * 2).check() == 0
    assert p.check(num_nets=1) == 0
    # nullable: the biases, and the projection's bias
    p.blocks[1][0].bias1 = p.blocks[1][0].bias2 = p.blocks[0][3].bias3 = None
    p.nets[0].proj_b = None
    assert p.check() == 0


def _edits():
    def blk(net, i, **kw):
        def edit(p):
            for k, v in kw.items():
                setattr(p.blocks[net][i], k, v)
        return edit

    def arena(**kw):
        def edit(p):
            for k, v in kw.items():
                setattr(p.arena, k, v)
        return edit

    def unfilled(p):
        p.items[2].px_off += 1

    def unfilled_stats(p):
        p.items[4].stats_off -= 16

    def no_blocks(p):
        p.nets[1].num_blocks = 0

    def elu_without_proj(p):
        p.nets[1].proj_w = None

    cases = [("w1 NULL", blk(0, 0, w1=None)), ("w2 NULL", blk(0, 55, w2=None)), ("w3 NULL", blk(1, 5, w3=None)),
             ("gamma without beta", blk(0, 7, beta2=None)), ("beta without gamma", blk(0, 7, gamma3=None)),
             ("norms partly given", blk(1, 2, gamma1=P, beta1=P)), ("dilation 0", blk(0, 1, dilation=0)),
             ("dilation 9", blk(1, 3, dilation=9)), ("dilation -1", blk(0, 9, dilation=-1)),
             ("eps < 0", blk(0, 2, eps=-1e-6)), ("eps NaN", blk(0, 2, eps=float("nan"))),
             ("SE vector NULL", blk(1, 0, se_b2=None)), ("odd weight pointer", blk(0, 0, w2=P + 1)),
             ("no blocks", no_blocks), ("in_elu without a projection", elu_without_proj),
             ("count 0", arena(count=0)), ("count -1", arena(count=-1)),
             ("items NULL", arena(items=None)), ("items_dev NULL", arena(items_dev=None)),
             ("stats NULL", arena(stats=None)), ("rows NULL", arena(rows=None)),
             ("stats misaligned", arena(stats=5 * P + 4)),
             ("offsets not the helper's", unfilled), ("stats offsets not the helper's", unfilled_stats)]
    for name in ("wide0", "wide1", "half0", "half1"):
        cases.append((f"{name} NULL", arena(**{name: None})))
        cases.append((f"{name} not 16-B aligned", arena(**{name: 9 * P + 8})))
    for a, b in (("wide0", "wide1"), ("wide1", "half0"), ("half0", "half1"), ("wide0", "half1")):
        cases.append((f"{a} == {b}", arena(**{a: 8 * P, b: 8 * P})))
    return cases


@pytest.mark.parametrize("name,edit", _edits(), ids=[n for n, _ in _edits()])
def test_refusals_are_einval(name, edit):
    p = Plan()
    edit(p)
    assert p.check() == EINVAL, name
    # the launching call refuses the same way, before it touches a dummy pointer
    which = ctypes.c_int32(7)
    assert _lib.load().di_head_body_batch(_lib.DI_BF16, p.nets, 2, ctypes.byref(p.arena), ctypes.byref(which),
                                          None) == EINVAL
    assert which.value == 7


def test_refusals_of_the_call_itself():
    lib = _lib.load()
    p = Plan()
    assert p.check(nets=None) == EINVAL and p.check(arena=None) == EINVAL
    assert p.check(num_nets=0) == EINVAL and p.check(num_nets=-2) == EINVAL
    assert p.check(dt=_lib.DI_F32) == EINVAL and p.check(dt=5) == EINVAL
    which = ctypes.c_int32(7)
    a = ctypes.byref(p.arena)
    assert lib.di_head_body_batch(_lib.DI_BF16, p.nets, 2, a, None, None) == EINVAL         # nowhere to answer
    assert lib.di_head_body_batch(_lib.DI_F32, p.nets, 2, a, ctypes.byref(which), None) == EINVAL
    assert lib.di_head_body_batch(_lib.DI_BF16, None, 2, a, ctypes.byref(which), None) == EINVAL
    assert lib.di_head_body_batch(_lib.DI_BF16, p.nets, 2, None, ctypes.byref(which), None) == EINVAL
    assert which.value == 7
    # an unfilled table (h and w alone), and more items than a batch holds
    q = Plan()
    q.items = head_items(SHAPES, fill=False)
    q.arena.items = ctypes.addressof(q.items)
    assert q.check() == EINVAL
    many = Plan([(2, 3)] * (_lib.DI_BATCH_MAX + 1))
    assert many.check() == ERANGE
    many.arena.count = _lib.DI_BATCH_MAX
    assert many.check() == 0
    # an item the convolutions' grids cannot hold: the 3x3 kernel's 65535 tile rows
    assert Plan([(16 * 65535 + 1, 1)]).check() == ERANGE


def test_logits_refusals_before_a_launch():
    lib = _lib.load()
    items = head_items(SHAPES)
    ok = dict(dt=_lib.DI_BF16, x=P, weight=2 * P, bias=3 * P, items=items, items_dev=4 * P, count=len(SHAPES),
              y=5 * P + 2)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.di_head_logits_batch(a["dt"], a["x"], a["weight"], a["bias"], a["items"], a["items_dev"],
                                        a["count"], a["y"], None)

    for kw in (dict(dt=_lib.DI_F32), dict(x=None), dict(x=P + 8), dict(weight=None), dict(weight=2 * P + 2),
               dict(bias=3 * P + 1), dict(y=None), dict(y=5 * P + 1), dict(y=P), dict(items=None),
               dict(items_dev=None), dict(count=0), dict(items=head_items(SHAPES, fill=False))):
        assert call(**kw) == EINVAL, kw
    many = head_items([(2, 3)] * (_lib.DI_BATCH_MAX + 1))
    assert call(items=many, count=len(many)) == ERANGE


def test_ctypes_structs_match_header():
    P8, F, I = ctypes.c_void_p, ctypes.c_float, ctypes.c_int32
    for cls, name, types, size in (
            (_lib.DiHeadBlock, "di_head_block", [P8] * 16 + [F, I], 16 * 8 + 8),
            (_lib.DiHeadNet, "di_head_net", [P8, P8, ctypes.POINTER(_lib.DiHeadBlock), I, I], 3 * 8 + 8),
            (_lib.DiHeadArena, "di_head_arena", [P8] * 8 + [I], 8 * 8 + 8)):
        assert [f for f, _ in cls._fields_] == _declared_struct_fields(name), name
        assert [t for _, t in cls._fields_] == types, name
        assert ctypes.sizeof(cls) == size, name
    decl = _declared_arg_counts()
    for fn, n in (("di_head_body_batch", 6), ("di_head_body_batch_check", 4), ("di_head_logits_batch", 9)):
        assert decl[fn] == n == len(_lib._SIGS[fn][0]), fn
    assert _lib.load().di_abi_version() == _lib.ABI_VERSION == 8


def test_plan_of_a_cpu_head():
    """62 blocks with the model's dilations; norms on the first ResNet only; the plan passes the C
    check with its own (host) pointers and a dummy arena, and notices a written parameter."""
    from deepinteract_amd.head import HeadBodyPlan, ResNet2DInputWithOptAttention
    head = ResNet2DInputWithOptAttention()
    plan = HeadBodyPlan(head)
    assert plan.num_blocks == 62 and [len(b) for b in plan.blocks] == [56, 6]
    assert plan.dilations == [1, 2, 4, 8] * 14 + [1, 2, 4, 8, 1, 1]
    assert [n.num_blocks for n in plan.nets] == [56, 6] and [n.in_elu for n in plan.nets] == [0, 1]
    assert all(n.proj_w and n.proj_b for n in plan.nets)
    assert all(b.gamma1 and b.beta3 and not b.bias1 and b.bias3 for b in plan.blocks[0])
    assert all(not b.gamma1 and not b.beta3 and b.bias1 and b.bias2 and b.bias3 for b in plan.blocks[1])
    assert plan.blocks[0][5].w2 == head.base_resnet._modules["resnet_base_resnet_1_2_conv2d_2"].weight.data_ptr()
    assert abs(plan.blocks[0][0].eps - 1e-6) < 1e-12
    dummy = Plan()
    assert _lib.load().di_head_body_batch_check(_lib.DI_BF16, plan.nets, 2, ctypes.byref(dummy.arena)) == 0
    assert not plan.stale()
    with torch.no_grad():
        head.phase2_resnet._modules["resnet_bin_resnet_extra1_se_block"].linear2.bias.add_(1.0)
    assert plan.stale()
    assert not HeadBodyPlan(head).stale()
    # the module's own plan: kept while fresh, rebuilt after a write, not carried into a copy
    import copy
    first = head.plan()
    assert head.plan() is first and head.plan(check="head") is first
    with torch.no_grad():
        head.base_resnet._modules["resnet_base_resnet_0_1_conv2d_1"].weight.mul_(0.5)
    assert first.stale("head") and head.plan(check="head") is not first
    assert copy.deepcopy(head)._plan is None


def test_litgini_head_body_option():
    from deepinteract_amd.modules import LitGINI
    assert LitGINI().head_body == "python"
    with pytest.raises(ValueError):
        LitGINI(head_body="native")                               # the default fp32 torch head
    with pytest.raises(ValueError):
        LitGINI(head_dtype=torch.bfloat16, head_body="native")    # bf16, but MIOpen convolutions
    with pytest.raises(ValueError):
        LitGINI(head_dtype=torch.bfloat16, head_convs="hip", head_body="c")
    for n in (0, 4):
        m = LitGINI(dtype="bf16", head_dtype=torch.bfloat16, head_convs="hip", head_batch=n, head_body="native")
        assert m.head_body == "native" and m.head_batch == n
    m = LitGINI(dtype="bf16", head_dtype=torch.bfloat16, head_convs="hip", head_body="native")
    assert m._head_chunks([(5, 5), (6, 6), (7, 7)]) == [[0], [1], [2]]   # head_batch=0: chunks of one
