"""fp64 restatement of the post-norm encoder layer and of the SWFormer block as TRAINED (point_transformer_layer.py:289-298,
314-339): plain torch on the CPU, differentiable, no call into the library.  The attention core is attn_ref.reference (ragged
windows from the CSR, optional dropout factors per (window, head)); DropPath enters as per-row factors mask / keep_prob.
Parameters come as a dict keyed like the modules' state_dict.  test_layer_ref.py holds it to oracle.window.encoder_layer, the
padded-window restatement every golden file was made with; test_gpu_encoder_layer.py holds the HIP path to it."""
import torch
import torch.nn.functional as F

from attn_ref import reference
from dropout_ref import dropout_factors

LN_EPS = 1e-5  # nn.LayerNorm's default, the value of EncoderLayer.norm1 / norm2

PARAM_NAMES = ("win_attn.self_attn.in_proj_weight", "win_attn.self_attn.in_proj_bias", "win_attn.self_attn.tau",
               "win_attn.self_attn.out_proj.weight", "win_attn.self_attn.out_proj.bias", "norm1.weight", "norm1.bias",
               "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "norm2.weight", "norm2.bias")


def keep_factors(wi, heads, p, seed):
    """{(window, head): [n, n] float64 factors 0 or 1 / keep_prob} of the attention dropout on the window index ``wi`` (the
    kernels' counter-based mask restated on the host, dropout_ref.py); None when p == 0."""
    if p <= 0.0:
        return None
    counts = wi.win_count[: wi.n_windows].cpu().tolist()
    return {(w, h): torch.from_numpy(dropout_factors(p, seed, w, h, n)) for w, n in enumerate(counts) for h in range(heads)}


def encoder_layer(x, pos, p, prefix, heads, wi, tau_min=0.01, keep=None, s1=None, s2=None, eps=LN_EPS, taps=None):
    """x2 of one layer.  keep: attention-dropout factors (keep_factors) or None; s1 / s2: per-row DropPath factors [m] or None.
    taps: optional dict that receives the intermediate tensors (qk, v, o, a, x1, h, m) for locating a disagreement."""
    c = x.shape[1]
    at = prefix + "win_attn.self_attn."
    w_in, b_in = p[at + "in_proj_weight"], p[at + "in_proj_bias"]
    qk = F.linear(x + pos, w_in[: 2 * c], b_in[: 2 * c])
    v = F.linear(x, w_in[2 * c:], b_in[2 * c:])
    o = reference(qk, v, p[at + "tau"], tau_min, heads, wi, keep).to(x.dtype)  # (float32 inputs: the float32 yardstick)
    a = F.linear(o, p[at + "out_proj.weight"], p[at + "out_proj.bias"])
    n1 = F.layer_norm(a, (c,), p[prefix + "norm1.weight"], p[prefix + "norm1.bias"], eps)
    x1 = x + (n1 if s1 is None else s1[:, None] * n1)
    h = F.linear(x1, p[prefix + "mlp.fc1.weight"], p[prefix + "mlp.fc1.bias"])
    g = 0.5 * h * (1.0 + torch.erf(h * 2.0 ** -0.5))  # the exact GELU
    m = F.linear(g, p[prefix + "mlp.fc2.weight"], p[prefix + "mlp.fc2.bias"])
    n2 = F.layer_norm(m, (c,), p[prefix + "norm2.weight"], p[prefix + "norm2.bias"], eps)
    x2 = x1 + (n2 if s2 is None else s2[:, None] * n2)
    if taps is not None:
        taps.update(qk=qk, v=v, o=o, a=a, x1=x1, h=h, m=m)
    return x2


def block(x, pos, index, p, depth, heads, keeps, scales, prefix="", tau_min=0.01):
    """SWFormerBlock: layer i on shift 0 if i < depth // 2 else 1 (pos[shift], index[shift]), with the attention-dropout
    factors keeps[i] and the DropPath factors scales[2 * i], scales[2 * i + 1] (entries may be None; scales None = none)."""
    for i in range(depth):
        s = 0 if i < depth // 2 else 1
        s1, s2 = (None, None) if scales is None else (scales[2 * i], scales[2 * i + 1])
        x = encoder_layer(x, pos[s], p, f"{prefix}layers.{i}.", heads, index[s], tau_min,
                          None if keeps is None else keeps[i], s1, s2)
    return x
