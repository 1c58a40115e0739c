"""The encoder layer AS TRAINED (ops._EncoderLayerFn through swformer.EncoderLayer / SWFormerBlock: attention dropout, per-row
DropPath inside both LayerNorm + residual passes, saved GELU derivative, residual gradients riding in GEMM epilogues) and its
inference routes against layer_ref.py, an fp64 restatement that calls nothing of the library (test_layer_ref.py holds it to the
padded-window oracle).  Every output row, dx and every one of the 13 parameter gradients is compared.

Window set: 1, 2, 16, 17, 33, 100, 129, 300 tokens = 598 rows (no multiple of 16 / 32 / 128), windows on both sides of the
16 / 32 / 128-token tile and chunk edges and one single-token window.

Bars (|got - ref|max <= bar * max(1, |ref|max)) start from the ones this project already holds the same arithmetic to: forward
3e-4 (golden block bar, tests/test_gpu_parity.py), dx and every non-tau gradient 5e-4 (whole-model median bar of
test_every_parameter_gradient_matches_oracle_autograd; six split-bf16 GEMMs and two LayerNorm backward passes in a chain), tau
2e-3 (attention tests), times max(1, 0.1 / tau) on the attention side of the sharp-softmax case (the rule of
test_attention_forward_and_backward_vs_fp64).  Every measurement below is under a quarter of its source bar, so the bar in force
is four times the measurement (MEASURED / bar_of; the source bar where that is lower -- the MLP-side gradients of case (c)): per case for y, dx and the parameter gradients; for tau four times the WORST
case, 1.1e-3 -- tau's gradient is ONE number summed over every (query, key, head) triple with heavy cancellation, its error
swings 100-fold from case to case (2.9e-06 .. 2.8e-04) where the other classes do not, and a benign reordering of that sum
must not fail a per-case figure.

Measured on the MI355X: worst |got - ref|max / max(1, |ref|max) per tensor class ("params" = the worst of the 12 non-tau
parameter gradients; 24 in the block).  f32 = the yardstick: the same layer_ref graph with the same inputs, mask and factors,
x / pos / parameters / upstream gradient cast to float32, run by torch on the CPU against its float64 self (as in
test_every_parameter_gradient_matches_oracle_autograd).  ``python tests/test_gpu_encoder_layer.py`` prints the yardstick
again; the measured figures are the FIGURE lines of ``pytest -s``.

  case                             y        dx    params       tau  |   f32: y        dx    params       tau
  (a) single node C=48  h=8  9.9e-06   2.7e-05   1.4e-05   2.4e-05  |  3.8e-07   5.3e-07   5.5e-07   9.7e-07
  (a) single node C=96  h=8  8.3e-06   1.4e-05   1.4e-05   2.9e-06  |  3.8e-07   6.5e-07   5.1e-07   3.3e-08
  (a) single node C=192 h=8  6.9e-06   9.9e-06   1.2e-05   2.4e-04  |  4.0e-07   5.0e-07   5.7e-07   1.6e-06
  (a) single node C=384 h=8  7.7e-06   8.5e-06   9.4e-06   7.6e-06  |  3.9e-07   4.8e-07   5.3e-07   4.6e-07
  (a) single node C=96  h=16 9.5e-06   6.1e-05   3.7e-05   2.9e-05  |  4.4e-07   7.4e-07   5.9e-07   4.7e-07
  (b) composed    C=48  h=8  9.9e-06   2.7e-05   1.4e-05   2.2e-05  |  as (a) C=48
  (b) composed    C=192 h=8  6.9e-06   9.7e-06   1.2e-05   2.8e-04  |  as (a) C=192
  (c) tau 0.02    C=96  h=8  5.7e-05   1.3e-04   1.3e-04   7.4e-05  |  1.5e-06   3.7e-06   3.7e-06   4.0e-06
  (e) block       C=96  h=8  8.6e-06   1.1e-05   1.4e-05   6.4e-05  |  (two layers of (a) C=96 h=8)

  (d) inference, y only         fast    module      grad  |   f32: y
  C=48  h=8                  1.1e-05   1.1e-05   1.1e-05  |  3.7e-07
  C=96  h=8                  7.1e-06   7.1e-06   7.1e-06  |  3.7e-07
  C=192 h=8                  5.7e-06   5.7e-06   5.7e-06  |  4.1e-07
  C=384 h=8                  5.7e-06   5.7e-06   5.7e-06  |  3.5e-07

The HIP path sits 15 - 40 times above float32 (split-bf16 products, ~2^-16 relative each) and 5 - 50 times under its source bars.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import layer_ref  # noqa: E402
from attn_ref import windows_of  # noqa: E402

SIZES = [1, 2, 16, 17, 33, 100, 129, 300]
SEED = 0x1234_5678_9ABC_DEF
ATTN_DROP, KEEP_PROB, TAU_MIN = 0.1, 0.8, 0.01
WIDTHS = [(48, 8), (96, 8), (192, 8), (384, 8)]

# where each class's bar comes from (module docstring): golden block bar, whole-model median bar (twice), attention tests
SOURCE_BARS = {"y": 3e-4, "dx": 5e-4, "param": 5e-4, "tau": 2e-3}
MEASURED = {  # case -> worst measured error of (y, dx, params, tau); (d): of y.  The table above, unrounded
    "a-48-8": (9.873e-06, 2.690e-05, 1.421e-05, 2.383e-05),
    "a-96-8": (8.271e-06, 1.367e-05, 1.369e-05, 2.860e-06),
    "a-192-8": (6.865e-06, 9.851e-06, 1.178e-05, 2.444e-04),
    "a-384-8": (7.700e-06, 8.480e-06, 9.418e-06, 7.567e-06),
    "a-96-16": (9.530e-06, 6.096e-05, 3.662e-05, 2.882e-05),
    "b-48-8": (9.873e-06, 2.694e-05, 1.416e-05, 2.246e-05),
    "b-192-8": (6.865e-06, 9.747e-06, 1.178e-05, 2.797e-04),
    "c-96-8": (5.716e-05, 1.315e-04, 1.269e-04, 7.413e-05),
    "d-48-fast": (1.067e-05,), "d-48-module": (1.065e-05,), "d-48-grad": (1.065e-05,),
    "d-96-fast": (7.070e-06,), "d-96-module": (7.070e-06,), "d-96-grad": (7.070e-06,),
    "d-192-fast": (5.670e-06,), "d-192-module": (5.670e-06,), "d-192-grad": (5.670e-06,),
    "d-384-fast": (5.716e-06,), "d-384-module": (5.716e-06,), "d-384-grad": (5.716e-06,),
    "e-96-8": (8.563e-06, 1.084e-05, 1.384e-05, 6.400e-05),
}
TAU_WORST = max(m[3] for m in MEASURED.values() if len(m) == 4)  # 2.797e-04: tau's bar is 4 x this in every case


def bar_of(case, cls, factor=1.0):
    """Four times the measurement where that is under the source bar (times ``factor``), the source bar otherwise; a case
    without a measurement is an error."""
    measured = TAU_WORST if cls == "tau" else MEASURED[case][("y", "dx", "param").index(cls)]
    return min(SOURCE_BARS[cls] * factor, 4.0 * measured)


# the tensors of the sharp-softmax case whose error the score scale amplifies: everything computed from the attention core's
# output or from what its backward returns (the MLP branch and norm2 sit behind LayerNorm 1 and keep the plain bars)
ATTENTION_SIDE = ("y", "dx", "win_attn.self_attn.in_proj_weight", "win_attn.self_attn.in_proj_bias", "win_attn.self_attn.tau",
                  "win_attn.self_attn.out_proj.weight", "win_attn.self_attn.out_proj.bias", "norm1.weight", "norm1.bias")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    out = windows_of(dev, SIZES)
    assert out.m == 598
    return out


@pytest.fixture(scope="module")
def refs():
    """fp64 references, computed once per (width, heads, tau, training) and shared by the cases; never modified."""
    return {}


def inputs(ws, c):
    """x, pos (scaled by 0.5: an input of the layer), upstream gradient: float64 draws, rounded to float32 for the GPU."""
    gen = torch.Generator().manual_seed(1000 + c)
    x = torch.randn(ws.m, c, generator=gen, dtype=torch.float64)
    pos = 0.5 * torch.randn(ws.m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(ws.m, c, generator=gen, dtype=torch.float64)
    return x, pos, g


def factors(ws):
    """Hand-built DropPath factors mask / keep_prob: ~20 % of the rows zero, the whole 17-token window dropped in s1, the
    single-token window dropped in s2, one row (of the 300-token window) dropped in both."""
    gen = torch.Generator().manual_seed(7)
    s1 = (torch.rand(ws.m, generator=gen) < KEEP_PROB).double() / KEEP_PROB
    s2 = (torch.rand(ws.m, generator=gen) < KEEP_PROB).double() / KEEP_PROB
    s1[ws.owner == SIZES.index(17)] = 0.0
    s2[ws.owner == SIZES.index(1)] = 0.0
    both = int(torch.nonzero(ws.owner == SIZES.index(300))[0])
    s1[both] = s2[both] = 0.0
    assert 0.1 < float((s1 == 0).double().mean()) < 0.35 and 0.1 < float((s2 == 0).double().mean()) < 0.35
    assert float(s1[ws.owner == SIZES.index(1)].min()) > 0.0  # the single-token window stays live in the attention branch
    return s1, s2


def make_layer(dev, c, heads, tau):
    from openseg3d_amd import swformer
    from oracle import params as oracle_params
    layer = swformer.EncoderLayer(c, heads, 2 * c, attn_drop=ATTN_DROP, drop_path_rate=1.0 - KEEP_PROB)
    oracle_params.fill_by_name(layer, seed=c + heads)
    with torch.no_grad():
        layer.win_attn.self_attn.tau.fill_(tau)
    assert sorted(k for k, _ in layer.named_parameters()) == sorted(layer_ref.PARAM_NAMES)
    assert layer.norm1.eps == layer.norm2.eps == layer_ref.LN_EPS
    return layer.to(dev)


def reference(refs, ws, layer, c, heads, tau, training):
    """(y, dx, {name: gradient}) of layer_ref.encoder_layer in fp64: with the dropout mask of (ATTN_DROP, SEED) and factors()
    when ``training``, without mask and factors otherwise."""
    key = (c, heads, tau, training)
    if key not in refs:
        x, pos, g = inputs(ws, c)
        p = {k: v.detach().cpu().double().requires_grad_() for k, v in layer.named_parameters()}
        x = x.requires_grad_()
        keep, (s1, s2) = (layer_ref.keep_factors(ws.wi, heads, ATTN_DROP, SEED), factors(ws)) if training else (None, (None, None))
        y = layer_ref.encoder_layer(x, pos, p, "", heads, ws.wi, TAU_MIN, keep, s1, s2)
        y.backward(g)
        refs[key] = (y.detach(), x.grad, {k: v.grad for k, v in p.items()})
    return refs[key]


def run_training(dev, ws, layer, c):
    """One training forward + backward of the layer on the GPU with the hand-built factors and the fixed seed."""
    x, pos, g = inputs(ws, c)
    s1, s2 = (s.float().to(dev) for s in factors(ws))
    layer.train().zero_grad(set_to_none=True)
    xg = x.float().to(dev).requires_grad_()
    y = layer(xg, pos.float().to(dev), ws.wi, scales=(s1, s2), seed=SEED)
    y.backward(g.float().to(dev))
    torch.cuda.synchronize()
    return y, xg.grad.clone(), {k: v.grad.clone() for k, v in layer.named_parameters()}


def rel_err(got, want):
    return float((got.detach().cpu().double() - want).abs().max()) / max(1.0, float(want.abs().max()))


def compare(label, got, want, sharp=1.0):
    """got / want: (y, dx, gradients by name).  Prints every figure, then asserts all of them: nothing is left out."""
    (y, dx, grads), (y_r, dx_r, grads_r) = got, want
    assert set(grads) == set(grads_r) and len(grads_r) % len(layer_ref.PARAM_NAMES) == 0
    rows = [("y", "y", y, y_r), ("dx", "dx", dx, dx_r)]
    rows += [(k, "tau" if k.endswith(".tau") else "param", grads[k], grads_r[k]) for k in grads_r]
    bad = []
    for name, cls, a, b in rows:
        assert a.shape == b.shape, name
        f = sharp if name in ATTENTION_SIDE else 1.0
        err, bar = rel_err(a, b), bar_of(label, cls, f)
        print(f"FIGURE {label} {name} class={cls} err={err:.3e} bar={bar:.3e} refmax={float(b.abs().max()):.3e}")
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, (label, bad)


@pytest.mark.parametrize("c,heads", WIDTHS + [(96, 16)])
def test_training_layer_single_node_vs_fp64(dev, ws, refs, c, heads):
    """(a) The layer as one autograd node, attention dropout 0.1 and DropPath factors in force: y, dx and all 13 parameter
    gradients against fp64 with the same mask and factors; a second run is bit-identical."""
    layer = make_layer(dev, c, heads, 0.3)
    y, dx, grads = run_training(dev, ws, layer, c)
    assert "EncoderLayerFn" in type(y.grad_fn).__name__
    compare(f"a-{c}-{heads}", (y, dx, grads), reference(refs, ws, layer, c, heads, 0.3, True))
    y2, dx2, grads2 = run_training(dev, ws, layer, c)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


@pytest.mark.parametrize("c,heads", [(48, 8), (192, 8)])
def test_training_layer_composed_modules_vs_fp64(dev, ws, refs, monkeypatch, c, heads):
    """(b) The same with the layer composed from its modules: that path is held to fp64 too, not only to its sibling."""
    from openseg3d_amd import swformer
    monkeypatch.setattr(swformer, "FUSED_LAYER", False)
    layer = make_layer(dev, c, heads, 0.3)
    y, dx, grads = run_training(dev, ws, layer, c)
    assert "EncoderLayerFn" not in type(y.grad_fn).__name__
    compare(f"b-{c}-{heads}", (y, dx, grads), reference(refs, ws, layer, c, heads, 0.3, True))


def test_training_layer_sharp_softmax_vs_fp64(dev, ws, refs):
    """(c) tau = 0.02: the online-maximum regime of the attention kernels inside the training layer."""
    c, heads, tau = 96, 8, 0.02
    layer = make_layer(dev, c, heads, tau)
    y, dx, grads = run_training(dev, ws, layer, c)
    assert "EncoderLayerFn" in type(y.grad_fn).__name__
    compare(f"c-{c}-{heads}", (y, dx, grads), reference(refs, ws, layer, c, heads, tau, True),
            sharp=max(1.0, 0.1 / tau))


def record_calls(monkeypatch):
    """Names of the library entry points called from here on."""
    from openseg3d_amd import _lib
    names, call = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", recording)
    return names


@pytest.mark.parametrize("c,heads", WIDTHS)
def test_inference_layer_vs_fp64(dev, ws, refs, monkeypatch, c, heads):
    """(d) Inference (eval, no mask, no factors) against fp64, by every route the layer has:
      * "fast": the node's inference forward -- ops._EncoderLayerFn.forward with nothing to keep: x + pos summed on the
        in-projection's A operand (seg3d_linear_fwd_sum), out-projection / fc2 + LayerNorm + residual in one launch each
        (seg3d_linear_layernorm_fwd) up to C = 192, apart at 384; the launches are recorded, so this route IS the one measured;
      * "module": swformer.EncoderLayer under no_grad, i.e. what a model runs today;
      * "grad": the module in eval mode with grad enabled (single node, nothing dropped).
    FINDING (recorded in DESIGN.md, "Inference fast paths of the encoder layer"; not changed here): a model never takes the
    "fast" route.  seg3d_linear_layernorm_fwd is unreachable from the module whatever the parameters' state: EncoderLayer.forward
    enters _EncoderLayerFn only with grad enabled and x.requires_grad, where ``live`` is always True, and _linear_layernorm has
    no other caller.  seg3d_linear_fwd_sum is reached only through the composed path with FROZEN parameters: inside a
    Function's forward ctx.needs_input_grad reports the inputs' requires_grad whatever the grad mode, so under no_grad
    ``not any(ctx.needs_input_grad)`` is still False for nn.Parameter inputs.  All three routes meet the same bar."""
    from openseg3d_amd import ops
    assert ops.LINEAR_LN_FUSED and ops.INPROJ_SUM
    layer = make_layer(dev, c, heads, 0.3).eval()
    x, pos, _ = inputs(ws, c)
    xg, pg = x.float().to(dev), pos.float().to(dev)
    y_ref = reference(refs, ws, layer, c, heads, 0.3, False)[0]
    at, mlp = layer.win_attn.self_attn, layer.mlp
    names = record_calls(monkeypatch)
    with torch.no_grad():
        meta = (heads, at.tau_min, ws.wi, layer.norm1.eps, layer.norm2.eps, None, None, 0.0, 0)
        y_fast = ops._EncoderLayerFn.forward(ops._Ctx(*[False] * 16), xg, pg, at.in_proj_weight, at.in_proj_bias, at.tau,
                                             at.out_proj.weight, at.out_proj.bias, layer.norm1.weight, layer.norm1.bias,
                                             mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, layer.norm2.weight,
                                             layer.norm2.bias, meta)
        fast = list(names)
        y_mod = layer(xg, pg, ws.wi)
    assert fast.count("seg3d_linear_fwd_sum") == 1
    assert fast.count("seg3d_linear_layernorm_fwd") == (2 if c <= 192 else 0)
    assert fast.count("seg3d_layernorm_fwd") == (0 if c <= 192 else 2)
    y_grad = layer(xg.clone().requires_grad_(), pg, ws.wi)
    assert "EncoderLayerFn" in type(y_grad.grad_fn).__name__
    bad = []
    for route, y in (("fast", y_fast), ("module", y_mod), ("grad", y_grad)):
        err, bar = rel_err(y, y_ref), bar_of(f"d-{c}-{route}", "y")
        print(f"FIGURE d-{c}-{route} y class=y err={err:.3e} bar={bar:.3e} refmax={float(y_ref.abs().max()):.3e}")
        if not err <= bar:
            bad.append((route, err, bar))
    assert not bad, bad


def test_block_wiring_vs_fp64(dev, monkeypatch):
    """(e) SWFormerBlock in training: layer 0 on the unshifted windows with seed + 0 and no DropPath (rate 0: its rows of the
    block's draw are never read -- they are overwritten with NaN here), layer 1 on the shifted windows with seed + 1 and the
    factors scales[2], scales[3] of the recorded draw."""
    from openseg3d_amd import scene, swformer
    from oracle import params as oracle_params
    c, heads, depth, seed = 96, 8, 2, 0x0BAD_5EED_0123_4567
    part = swformer.SparseWindowPartitionLayer({0: {"max_tokens": 800, "batching_range": [0, 100000]}}, [10, 10, 8],
                                               [360.0, 360.0, 16.0])
    pts = scene.make_small_scene(5, 9000, extent=12.0)
    coords = np.unique(np.floor((pts[:, :3] - pts[:, :3].min(0)) / 0.4).astype(np.int32)[:, ::-1], axis=0)
    coords = torch.from_numpy(np.concatenate([np.zeros((coords.shape[0], 1), np.int32), coords], 1)).to(dev)
    plan = part.plan(coords, 1, c)
    assert not torch.equal(plan.index[0].tok, plan.index[1].tok)  # both shifts are real
    m = coords.shape[0]
    blk = swformer.SWFormerBlock(c, heads, depth=depth, drop_path=[0.0, 0.3])
    oracle_params.fill_by_name(blk, seed=5)
    blk = blk.to(dev).train()
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)

    recorded, draw = [], blk.drop_path_scales

    def recording_draw(feats):
        s = draw(feats)
        recorded.append(s.clone())
        s[:2] = float("nan")  # layer 0 has rate 0: whatever it read of these rows would show
        return s

    monkeypatch.setattr(blk, "drop_path_scales", recording_draw)
    monkeypatch.setattr(swformer, "attention_dropout_seed", lambda: seed)
    xg = x.float().to(dev).requires_grad_()
    with torch.random.fork_rng(devices=[dev]):  # the block's DropPath draw comes from the device generator: the same draw in
        torch.manual_seed(0)                    # every run, and the generators of the tests after this one left as they were
        y = blk({"voxel_features": xg, "plan": plan})
    assert "EncoderLayerFn" in type(y.grad_fn).__name__
    y.backward(g.float().to(dev))
    torch.cuda.synchronize()
    assert len(recorded) == 1 and tuple(recorded[0].shape) == (2 * depth, m)
    s = recorded[0].cpu().double()
    zeros = (s[2:] == 0).double().mean(1)
    assert bool(((zeros > 0.2) & (zeros < 0.4)).all()) and not torch.equal(s[2], s[3])

    p = {k: v.detach().cpu().double().requires_grad_() for k, v in blk.named_parameters()}
    keeps = [layer_ref.keep_factors(plan.index[0 if i < depth // 2 else 1], heads, ATTN_DROP, seed + i) for i in range(depth)]
    x_r = x.requires_grad_()
    y_r = layer_ref.block(x_r, [t.cpu().double() for t in plan.pos], plan.index, p, depth, heads, keeps, [None, None, s[2], s[3]])
    y_r.backward(g)
    compare("e-96-8", (y, xg.grad, {k: v.grad for k, v in blk.named_parameters()}),
            (y_r.detach(), x_r.grad, {k: v.grad for k, v in p.items()}))


def float32_yardstick(ws, c, heads, tau, training):
    """Worst error per class (y, dx, params, tau) of layer_ref in float32 on the CPU against its float64 self: same inputs,
    mask and factors as the cases above (the f32 columns of the module docstring)."""
    layer = make_layer(torch.device("cpu"), c, heads, tau)
    y_r, dx_r, grads_r = reference({}, ws, layer, c, heads, tau, training)
    x, pos, g = inputs(ws, c)
    p = {k: v.detach().clone().requires_grad_() for k, v in layer.named_parameters()}
    x = x.float().requires_grad_()
    keep = s1 = s2 = None
    if training:
        keep = {k: v.float() for k, v in layer_ref.keep_factors(ws.wi, heads, ATTN_DROP, SEED).items()}
        s1, s2 = (s.float() for s in factors(ws))
    layer_ref.encoder_layer(x, pos.float(), p, "", heads, ws.wi, TAU_MIN, keep, s1, s2).backward(g.float())
    errs = {k: rel_err(v.grad, grads_r[k]) for k, v in p.items()}
    with torch.no_grad():
        y = layer_ref.encoder_layer(x, pos.float(), p, "", heads, ws.wi, TAU_MIN, keep, s1, s2)
    return (rel_err(y, y_r), rel_err(x.grad, dx_r), max(e for k, e in errs.items() if not k.endswith(".tau")),
            max(e for k, e in errs.items() if k.endswith(".tau")))


if __name__ == "__main__":  # the window index comes from the partition kernel: needs the GPU like the tests
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    windows = windows_of(torch.device("cuda:0"), SIZES)
    for c_, heads_, tau_, training_ in ([(c, h, 0.3, True) for c, h in WIDTHS + [(96, 16)]] + [(96, 8, 0.02, True)]
                                        + [(c, h, 0.3, False) for c, h in WIDTHS]):
        print(f"f32 yardstick C={c_} heads={heads_} tau={tau_} training={training_}: y %.1e dx %.1e params %.1e tau %.1e"
              % float32_yardstick(windows, c_, heads_, tau_, training_))
