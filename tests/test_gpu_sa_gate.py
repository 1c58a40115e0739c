"""The one-channel submanifold conv and the fused SALayer gate on the device (csrc/sa_gate.hip): bit for bit against
the library's host twins wherever no expf is involved (the logits; dx, dw and dbias of the plain conv, whose ds is the
incoming gradient), bit for bit against a second run for everything, and within the float64 bounds of tests/sa_ref.py.
Then SALayer, SparseBasicBlock(with_sa=True) under both backbones' names and the block with squeeze-excite alone on one
shared 300-site case."""
from functools import partial

import numpy as np
import pytest
import torch

import sa_ref as ref
from sa_ref import CHANNELS, ROW_COUNTS, ROWS, make_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


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


def _device_vs_host(tag, case, refs, gate):
    got = ref.run_ops(case, gate, "cuda:0")
    again = ref.run_ops(case, gate, "cuda:0")
    host = ref.run_ops(case, gate, "cpu")
    assert set(got) == set(host)
    for name in got:
        assert ref.same_bits(got[name], again[name]), f"{tag} {name}: two device runs differ"
    exact = ("s",) if gate else ("s", "dx", "dw", "db")  # no expf on the way
    for name in exact:
        assert ref.same_bits(got[name], host[name]), f"{tag} {name}: device and host twin differ"
    ref.check_all(tag, got, refs[gate])


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("m", ROW_COUNTS)
def test_device_against_host_twin_and_fp64(cases, m, c):
    """Every lane layout (C = 4: one lane; 32, 96, 192: power-of-two groups filled; 48: 12 of 16 lanes; 384: two passes) at
    every row count (wave tails; one, two, several weight-gradient blocks, a short last block)."""
    case, refs = cases(m, c)
    for gate in (False, True):
        _device_vs_host(f"M={m} C={c} gate={gate}", case, refs, gate)


@pytest.mark.parametrize("sites,m", [("solid", 216), ("isolated", 65), ("batch", 216)])
@pytest.mark.parametrize("c", [4, 48])
def test_site_sets(cases, sites, m, c):
    """A solid 6 x 6 x 6 cube (27 neighbours inside, 8 at the corners), centre-only rows, and two samples whose blocks
    touch in coordinates but not in batch index (ref.table asserts that no neighbour crosses)."""
    case, refs = cases(m, c, sites)
    for gate in (False, True):
        _device_vs_host(f"{sites} C={c} gate={gate}", case, refs, gate)


def test_saturated_logits():
    ref.saturation_check("cuda:0")


@pytest.mark.parametrize("gate", [False, True], ids=["subm_dot", "sa_gate"])
def test_needs_input_grad_subsets(cases, gate):
    case, _ = cases(ROWS + 1, 48)
    d = "cuda:0"
    full = ref.run_ops(case, gate, d)
    only_x = ref.run_ops(case, gate, d, need_w=False, need_b=False)
    only_w = ref.run_ops(case, gate, d, need_x=False, need_b=False)
    no_bias = ref.run_ops(case, gate, d, bias=False)
    assert set(only_x) & {"dx", "dw", "db"} == {"dx"} and set(only_w) & {"dx", "dw", "db"} == {"dw"}
    assert ref.same_bits(only_x["dx"], full["dx"]) and ref.same_bits(only_w["dw"], full["dw"])
    assert "db" not in no_bias
    assert ref.same_bits(no_bias["dx"], full["dx"]) and ref.same_bits(no_bias["dw"], full["dw"])
    if not gate:
        only_b = ref.run_ops(case, gate, d, need_x=False, need_w=False)
        assert set(only_b) & {"dx", "dw", "db"} == {"db"} and ref.same_bits(only_b["db"], full["db"])


def test_unaligned_input_is_rejected(dev):
    """The header: x is read as 16-byte vectors and must be 16-byte aligned; an x that starts 4 bytes after such a boundary
    is SEG3D_EINVAL (nothing is launched), and the same rows at an aligned address are accepted."""
    from openseg3d_amd import _lib, ops
    case = make_case(65, 8)
    nbr = torch.from_numpy(case["nbr"]).to(dev)
    w = torch.from_numpy(case["w"]).to(dev)
    buf = torch.zeros(65 * 8 + 8, device=dev)
    assert buf.data_ptr() % 16 == 0
    shifted = buf[1:1 + 65 * 8].view(65, 8)
    shifted.copy_(torch.from_numpy(case["x"]))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for call in (lambda t: ops.subm_dot(t, w, None, nbr), lambda t: ops.sa_gate(t, w, nbr)):
        with pytest.raises(_lib.Seg3dError):
            call(shifted)
        call(shifted.clone())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ layer level
C_LAYER = 32


@pytest.fixture(scope="module")
def layer_case(dev):
    """300 sites of a 6 x 6 x * block (raster order) with two samples, features and an upstream gradient, shared by the layer
    tests; the float64 SA step comes from ref.reference on the same table."""
    case = make_case(300, C_LAYER, seed=3)
    coords = case["coords"].copy()
    coords[:, 0] = (np.arange(300) >= 180).astype(np.int32)  # rows 0..179 (z < 5) and 180..299: two samples
    case["coords"], case["bs"] = coords, 2
    case["nbr"] = ref.table(coords, case["shape"])
    return case


def _tensor(case, dev, feats):
    from openseg3d_amd import spconv
    return spconv.SparseConvTensor(feats, torch.from_numpy(case["coords"]).to(dev), case["shape"], case["bs"])


def test_sa_layer_forward_backward(dev, layer_case):
    from openseg3d_amd import segformer
    case = layer_case
    refs = ref.reference(case, True)
    sa = segformer.SALayer(C_LAYER, indice_key="subm1").to(dev)
    with torch.no_grad():
        sa.conv.weight.copy_(torch.from_numpy(case["w"]))
    x = torch.from_numpy(case["x"]).to(dev).requires_grad_()
    xt = _tensor(case, dev, x)
    assert torch.equal(xt.level.subm().cpu(), torch.from_numpy(case["nbr"])), "device table differs from the oracle's"
    y = sa(xt).features
    y.backward(torch.from_numpy(case["dy"]).to(dev))
    got = {"y": y.detach().cpu().numpy(), "dx": x.grad.cpu().numpy(),
           "dw": sa.conv.weight.grad.cpu().numpy().reshape(27, C_LAYER)}
    ref.check_all("SALayer", got, refs)


def _sa_step_f64(f, w, nbr, identity):
    """relu(f * sigmoid(conv(f)) + identity) in float64 (torch autograd)."""
    s = ref.sc.apply_rulebook(f, nbr, w)
    return torch.relu(f * torch.sigmoid(s) + identity)


@pytest.mark.parametrize("backbone", ["segformer", "spnet"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_basic_block_with_sa(dev, layer_case, backbone, mode):
    """SparseBasicBlock(32, 32, with_sa=True) against the same block assembled from the existing modules (conv1, bn1 + ReLU,
    conv2, bn2 of the block itself, on the device) followed by the float64 SA step, + identity, ReLU.  Tolerances of the
    conv path: 1e-4 absolute for outputs and input gradients, 1e-4 * max(1, max |dw|) for weight gradients
    (tests/test_gpu_conv_tiled.py, tests/test_gpu_parity.py).  eval runs under no_grad and takes the fused conv-BN launches."""
    import importlib
    from openseg3d_amd import ops
    mod = importlib.import_module("openseg3d_amd." + backbone)
    case = layer_case
    torch.manual_seed(11)
    norm = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    block = mod.SparseBasicBlock(C_LAYER, C_LAYER, norm, torch.nn.ReLU(), indice_key="subm1", with_sa=True).to(dev)
    with torch.no_grad():
        for bn in (block.bn1, block.bn2):
            bn.running_mean.normal_(0, 0.1)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.1)
    nbr = case["nbr"]
    w_sa = block.sa.conv.weight.detach().cpu().double().requires_grad_()
    x = torch.from_numpy(case["x"]).to(dev)
    if mode == "eval":
        block.eval()
        with torch.no_grad():
            xt = _tensor(case, dev, x)
            assert block.conv1.fusable_with(block.bn1, xt) and block.conv2.fusable_with(block.bn2, xt)
            out = block(xt).features
            f = block.conv2.forward_bn_act(block.conv1.forward_bn_act(xt, block.bn1, relu=True), block.bn2, relu=False).features
        want = _sa_step_f64(f.cpu().double(), w_sa, nbr, x.cpu().double())
        err = float((out.cpu().double() - want.detach()).abs().max())
        print(f"{backbone} eval: max error {err:.3e}")
        assert err < 1e-4
        return
    block.train()
    momentum_state = {k: v.clone() for k, v in block.state_dict().items()}
    x1 = x.clone().requires_grad_()
    out = block(_tensor(case, dev, x1)).features
    seed = torch.from_numpy(case["dy"]).to(dev)
    out.backward(seed)
    got = {n: p.grad.clone() for n, p in block.named_parameters()}
    block.load_state_dict(momentum_state)  # the running statistics moved; same starting point for the assembled pass
    block.zero_grad()
    x2 = x.clone().requires_grad_()
    xt = _tensor(case, dev, x2)
    y = block.conv1(xt)
    y = y.replace_feature(ops.batch_norm_act(y.features, block.bn1, relu=True))
    y = block.conv2(y)
    f = ops.batch_norm_act(y.features, block.bn2, relu=False)
    f64 = f.detach().cpu().double().requires_grad_()
    x64 = x.cpu().double().requires_grad_()
    want = _sa_step_f64(f64, w_sa, nbr, x64)
    err = float((out.detach().cpu().double() - want.detach()).abs().max())
    want.backward(seed.cpu().double())
    f.backward(f64.grad.float().to(dev))  # through the existing modules
    dx_want = x2.grad.cpu().double() + x64.grad
    dx_err = float((x1.grad.cpu().double() - dx_want).abs().max())
    print(f"{backbone} train: out max error {err:.3e}, dx max error {dx_err:.3e}")
    assert err < 1e-4 and dx_err < 1e-4
    for n, p in block.named_parameters():
        want_g = w_sa.grad.reshape(p.shape) if n == "sa.conv.weight" else p.grad.cpu().double()
        g_err = float((got[n].cpu().double() - want_g).abs().max())
        print(f"  d {n}: max error {g_err:.3e}")
        assert g_err < 1e-4 * max(1.0, float(want_g.abs().max())), n


def test_basic_block_with_se_alone_keeps_the_separate_passes_in_eval(dev, layer_case):
    """SparseBasicBlock(32, 32, with_se=True) in eval() under no_grad is, bit for bit, the sequence assembled from its own
    modules: conv1, bn1 + ReLU, conv2, bn2 as passes of their own (no BatchNorm folded into the convs, although both convs
    could take it), squeeze-excite, + identity, ReLU -- what SparseUnet's conv3 / conv4 tails compute in inference."""
    from openseg3d_amd import ops, segformer
    case = layer_case
    torch.manual_seed(11)
    norm = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    block = segformer.SparseBasicBlock(C_LAYER, C_LAYER, norm, torch.nn.ReLU(), indice_key="subm1", with_se=True).to(dev)
    assert block.se is not None and block.sa is None
    with torch.no_grad():
        for bn in (block.bn1, block.bn2):
            bn.running_mean.normal_(0, 0.1)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.1)
    x = torch.from_numpy(case["x"]).to(dev)
    block.eval()
    with torch.no_grad():
        xt = _tensor(case, dev, x)
        assert block.conv1.fusable_with(block.bn1, xt) and block.conv2.fusable_with(block.bn2, xt)
        out = block(xt).features
        y = block.conv1(xt)
        y = y.replace_feature(ops.batch_norm_act(y.features, block.bn1, relu=True))
        y = block.conv2(y)
        f = ops.batch_norm_act(y.features, block.bn2, relu=False)
        f = block.se(f, y.indices[:, 0], y.level.sample_offsets())
        want = torch.relu(f + x)
    print(f"SE-only eval: max difference {float((out - want).abs().max()):.3e}")
    assert torch.equal(out, want)


@pytest.mark.parametrize("backbone", ["segformer", "spnet"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_with_sa_false_is_the_block_without_the_argument(dev, layer_case, backbone, mode):
    import importlib
    mod = importlib.import_module("openseg3d_amd." + backbone)
    case = layer_case
    norm = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    torch.manual_seed(7)
    a = mod.SparseBasicBlock(C_LAYER, C_LAYER, norm, torch.nn.ReLU(), indice_key="subm1").to(dev)
    b = mod.SparseBasicBlock(C_LAYER, C_LAYER, norm, torch.nn.ReLU(), indice_key="subm1", with_sa=False).to(dev)
    b.load_state_dict(a.state_dict())
    x = torch.from_numpy(case["x"]).to(dev)
    outs = []
    for block in (a, b):
        block.train(mode == "train")
        with torch.set_grad_enabled(mode == "train"):
            xi = x.clone().requires_grad_(mode == "train")
            out = block(_tensor(case, dev, xi)).features
            if mode == "train":
                out.backward(torch.from_numpy(case["dy"]).to(dev))
                outs.append((out.detach(), xi.grad, block.conv1.weight.grad, block.conv2.weight.grad))
            else:
                outs.append((out,))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
