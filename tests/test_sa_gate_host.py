"""The one-channel submanifold conv and the fused SALayer gate on CPU tensors (the library's _host twins, plain C++ in
the order of summation the header fixes) against the float64 reference and the derived bounds of tests/sa_ref.py, plus
the construction / state-dict surface: SubMConv3d(C, 1), SALayer, SparseBasicBlock(with_sa=True) of both backbones."""
from functools import partial

import numpy as np
import pytest
import torch

import sa_ref as ref
from sa_ref import CHANNELS, ROWS, make_case

# every C once per row count around the weight-gradient block, small counts with the narrow and the two-pass rows
HOST_SHAPES = [(0, 32), (1, 4), (63, 384), (64, 48), (65, 96), (ROWS - 1, 192), (ROWS, 32), (ROWS + 1, 48),
               (3 * ROWS + 5, 4), (3 * ROWS + 5, 96), (ROWS + 1, 384)]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(m, c, sites="solid", **kw):
        key = (m, c, sites, tuple(sorted(kw.items())))
        if key not in cache:
            case = make_case(m, c, sites, **kw)
            cache[key] = (case, {True: ref.reference(case, True), False: ref.reference(case, False)})
        return cache[key]
    return get


def test_site_sets_have_the_table_properties():
    """ref.table asserts centre, mirror and no neighbour across samples; here also the neighbour counts the cases rely on."""
    solid = make_case(216, 4)
    cnt = (solid["nbr"] >= 0).sum(0)
    assert cnt.max() == 27 and cnt.min() == 8
    iso = make_case(65, 4, "isolated")
    assert np.array_equal((iso["nbr"] >= 0).sum(0), np.ones(65, np.int64))
    two = make_case(0, 4, "batch")
    face = np.isin(two["coords"][:, 1], (2, 3))  # the layers where the two samples touch: nothing from across
    assert two["m"] == 216 and two["bs"] == 2 and (two["nbr"] >= 0).sum(0)[face].max() == 18


@pytest.mark.parametrize("m,c", HOST_SHAPES)
@pytest.mark.parametrize("gate", [False, True], ids=["subm_dot", "sa_gate"])
def test_host_twins_within_the_fp64_bounds(cases, m, c, gate):
    case, refs = cases(m, c)
    got = ref.run_ops(case, gate, "cpu")
    assert {"s", "dx", "dw"} <= set(got) and (gate or "db" in got) and (not gate or "y" in got)
    ref.check_all(f"host M={m} C={c}", got, refs[gate])
    again = ref.run_ops(case, gate, "cpu")
    for name in got:
        assert ref.same_bits(got[name], again[name]), f"{name} differs between two calls"


@pytest.mark.parametrize("sites", ["isolated", "batch"])
@pytest.mark.parametrize("c", [4, 48])
def test_host_twins_on_the_other_site_sets(cases, sites, c):
    case, refs = cases(65, c, sites)
    for gate in (False, True):
        ref.check_all(f"host {sites} C={c} gate={gate}", ref.run_ops(case, gate, "cpu"), refs[gate])


@pytest.mark.parametrize("c", CHANNELS)
def test_fused_gate_equals_the_composition(cases, c):
    """ops.sa_gate against x * sigmoid(ops.subm_dot(x, w, None, nbr)): the saved logits are the same bits, outputs and
    gradients of both stay within the bounds."""
    from openseg3d_amd import ops
    case, refs = cases(ROWS + 1, c)
    fused = ref.run_ops(case, True, "cpu")
    x = torch.from_numpy(case["x"]).requires_grad_()
    w = torch.from_numpy(case["w"]).requires_grad_()
    s = ops.subm_dot(x, w, None, torch.from_numpy(case["nbr"]))
    assert ref.same_bits(fused["s"], s.detach().numpy().reshape(-1)), "saved logits differ from the plain conv's"
    y = x * torch.sigmoid(s)
    y.backward(torch.from_numpy(case["dy"]))
    comp = {"y": y.detach().numpy(), "dx": x.grad.numpy(), "dw": w.grad.numpy().reshape(27, c)}
    ref.check_all(f"fused C={c}", fused, refs[True])
    ref.check_all(f"composition C={c}", comp, refs[True])


def test_saturated_logits():
    ref.saturation_check("cpu")


@pytest.mark.parametrize("gate", [False, True], ids=["subm_dot", "sa_gate"])
def test_needs_input_grad_subsets(cases, gate):
    case, _ = cases(ROWS + 1, 48)
    full = ref.run_ops(case, gate, "cpu")
    only_x = ref.run_ops(case, gate, "cpu", need_w=False, need_b=False)
    only_w = ref.run_ops(case, gate, "cpu", need_x=False, need_b=False)
    no_bias = ref.run_ops(case, gate, "cpu", bias=False)
    assert set(only_x) & {"dx", "dw", "db"} == {"dx"} and set(only_w) & {"dx", "dw", "db"} == {"dw"}
    assert ref.same_bits(only_x["dx"], full["dx"]) and ref.same_bits(only_w["dw"], full["dw"])
    assert "db" not in no_bias
    # the bias enters s only: the gradients with respect to x and the weight do not see it
    assert ref.same_bits(no_bias["dx"], full["dx"]) and ref.same_bits(no_bias["dw"], full["dw"])
    if not gate:
        only_b = ref.run_ops(case, gate, "cpu", need_x=False, need_w=False)
        assert set(only_b) & {"dx", "dw", "db"} == {"db"} and ref.same_bits(only_b["db"], full["db"])


def test_rejected_arguments():
    """bfloat16 storage, a channel count outside the accepted set, and an x that starts 4 bytes after a 16-byte boundary
    (the header: rejected with SEG3D_EINVAL) raise the library's error."""
    from openseg3d_amd import _lib, ops
    case = make_case(65, 8)
    nbr = torch.from_numpy(case["nbr"])
    x, w = torch.from_numpy(case["x"]), torch.from_numpy(case["w"])
    with pytest.raises(_lib.Seg3dError):
        ops.sa_gate(x.bfloat16(), w, nbr)
    with pytest.raises(_lib.Seg3dError):
        ops.subm_dot(x[:, :6].contiguous(), w[..., :6].contiguous(), None, nbr)
    with pytest.raises(_lib.Seg3dError):
        ops.subm_dot(torch.zeros(65, 1028), torch.zeros(1, 3, 3, 3, 1028), None, nbr)
    buf = torch.zeros(65 * 8 + 8)
    off = ((4 - buf.data_ptr() % 16) // 4) % 4  # first element 4 bytes after a 16-byte boundary
    shifted = buf[off:off + 65 * 8].view(65, 8)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    with pytest.raises(_lib.Seg3dError):
        ops.subm_dot(shifted, w, None, nbr)
    with pytest.raises(_lib.Seg3dError):
        ops.sa_gate(shifted, w, nbr)
    assert _lib.query("seg3d_subm_dot_scratch_bytes", 3 * ROWS + 5, 48) >= 4 * (27 * 48 + 1) * 4
    assert _lib.query("seg3d_subm_dot_scratch_bytes", 10, 6) == 0


def test_construction_and_state_dict_keys():
    from openseg3d_amd import checkpoint, segformer, spconv, spnet
    conv = spconv.SubMConv3d(32, 1, 3, padding=1, bias=False)
    assert tuple(conv.weight.shape) == (1, 3, 3, 3, 32) and conv.bias is None
    assert tuple(spconv.SubMConv3d(32, 1, 3, padding=1, bias=True).bias.shape) == (1,)
    bn = torch.nn.BatchNorm1d(1).eval()
    feats = torch.zeros(4, 32)
    with torch.no_grad():
        assert conv.fusable_with(bn, spconv.SparseConvTensor(feats, torch.zeros(4, 4, dtype=torch.int32), [4, 4, 4], 1)) is False
    for bad in (partial(spconv.SubMConv3d, 32, 8, 3, padding=1), partial(spconv.SubMConv3d, 32, 17, 3, padding=1),
                partial(spconv.SubMConv3d, 6, 1, 3, padding=1), partial(spconv.SubMConv3d, 32, 1, 3, padding=0),
                partial(spconv.SparseConv3d, 32, 1, 3, stride=2, padding=1), partial(spconv.SparseInverseConv3d, 32, 1, 3)):
        with pytest.raises(NotImplementedError):
            bad()
    sa = segformer.SALayer(32, indice_key="subm1")
    assert {k: tuple(v.shape) for k, v in sa.state_dict().items()} == {"conv.weight": (1, 3, 3, 3, 32)}
    assert spnet.SALayer is segformer.SALayer
    assert spnet.SparseBasicBlock is segformer.SparseBasicBlock and spnet.UpBlock is segformer.UpBlock
    norm = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    # the two reference classes order indice_key and with_se differently: the options are keyword-only
    with pytest.raises(TypeError):
        segformer.SparseBasicBlock(32, 32, norm, torch.nn.ReLU(), "subm1")
    with pytest.raises(TypeError):
        segformer.SparseBasicBlock(32, 32, norm, torch.nn.ReLU(), True)
    for mod in (segformer, spnet):
        block = mod.SparseBasicBlock(32, 32, norm, torch.nn.ReLU(), indice_key="subm1", with_sa=True)
        assert tuple(block.state_dict()["sa.conv.weight"].shape) == (1, 3, 3, 3, 32)
        plain = mod.SparseBasicBlock(32, 32, norm, torch.nn.ReLU(), indice_key="subm1")
        assert plain.sa is None and plain.se is None
        assert set(block.state_dict()) - set(plain.state_dict()) == {"sa.conv.weight"}
        # a checkpoint that stores the spconv-1.x layout [3, 3, 3, Cin, 1] loads into sa.conv.weight
        sd = {k: v.clone() for k, v in block.state_dict().items()}
        want = torch.randn(1, 3, 3, 3, 32)
        sd["sa.conv.weight"] = want.permute(1, 2, 3, 4, 0).contiguous()
        assert torch.equal(checkpoint.convert_spconv_state_dict(sd, block)["sa.conv.weight"], want)
    both = segformer.SparseBasicBlock(32, 32, norm, torch.nn.ReLU(), with_se=True, with_sa=True)
    assert {"se.fc.0.weight", "se.fc.2.weight", "sa.conv.weight"} <= set(both.state_dict())
