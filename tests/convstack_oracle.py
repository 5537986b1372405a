"""TEST INFRASTRUCTURE ONLY.  One ConvStack call (Engine.convstack / engine_bwd._convstack_bwd: four 3x3 convolutions, each with BatchNorm2d and ReLU,
the 40 F -> 256 Linear without bias, BatchNorm1d, ReLU, dropout) restated in plain torch on the CPU, in float64 or float32: what
tests/test_gpu_convstack_call.py holds every path of the call to, tensor by tensor.  Checked against oracle/model_ref.convstack_forward and
torch.nn.BatchNorm{1,2}d by tests/test_convstack_oracle_cpu.py; shaped like tests/encoder_oracle.py.

What the call exposes beyond model_ref.convstack_forward: the four pre-BatchNorm outputs in the device's (B, T, C, F) layout, every BatchNorm's
(mean, invstd, scale, shift) with scale = gamma invstd and shift = beta - mean scale, the operand ranges (per-channel max |y| and the activation
bound), the Linear's output z, the updated buffers -- and the ReLU DECISIONS: the gradients are discontinuous where a pre-activation crosses the
threshold, so `gradients` can be told the decisions (masks) instead of taking them itself, and `forward` returns per layer the normalised
pre-activation pre_i = xhat + beta / gamma = bn_i(y_i) / gamma, whose distance from 0 is the distance from the threshold in standard deviations
of the channel.

No device, no ctypes; imports nothing of the product package."""
import torch

LAYERS = (1, 2, 3, 4)
BN_NAMES = tuple(f"convstack.bn{i}" for i in LAYERS) + ("convstack.out_bn",)
CONV_PARAMS = [f"convstack.conv{i}.weight" for i in LAYERS] + [f"convstack.bn{i}.{w}" for i in LAYERS for w in ("weight", "bias")] + [
    "convstack.out.weight", "convstack.out_bn.weight", "convstack.out_bn.bias"]                  # the 15 tensors, by the reference's state_dict names
BUFFERS = tuple(f"{n}.{b}" for n in BN_NAMES for b in ("running_mean", "running_var", "num_batches_tracked"))
BN_PARTS = ("mean", "invstd", "scale", "shift")
EPS, MOMENTUM, KEEP = 1e-5, 0.1, 0.8


def convstack_tensors(state):
    """(the 15 parameters, the 15 buffers) out of a state dict."""
    return {k: state[k] for k in CONV_PARAMS}, {k: state[k] for k in BUFFERS}


def _short(name):
    return name[len("convstack."):]


def _bn(res, new_buffers, y, P, buffers, name, dims, shape, training, dtype):
    """BatchNorm over `dims` of y; records the quadruple under the short name, the updated buffers in training.  Returns (u = bn(y), pre = u / gamma)."""
    gamma, beta = P[name + ".weight"], P[name + ".bias"]
    if training:
        n = y.numel() // gamma.numel()
        mean = y.mean(dim=dims)
        var = ((y - mean.view(shape)) ** 2).mean(dim=dims)                   # biased: what normalises
        with torch.no_grad():
            rm, rv = buffers[name + ".running_mean"].to(dtype), buffers[name + ".running_var"].to(dtype)
            new_buffers[name + ".running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
            new_buffers[name + ".running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * var * (n / (n - 1))          # unbiased: rows = 1 is undefined (torch raises)
            new_buffers[name + ".num_batches_tracked"] = buffers[name + ".num_batches_tracked"] + 1
    else:
        mean, var = buffers[name + ".running_mean"].to(dtype), buffers[name + ".running_var"].to(dtype)
    invstd = 1 / torch.sqrt(var + EPS)
    xhat = (y - mean.view(shape)) * invstd.view(shape)
    u = xhat * gamma.view(shape) + beta.view(shape)
    with torch.no_grad():
        scale = gamma * invstd
        for k, v in zip(BN_PARTS, (mean, invstd, scale, beta - mean * scale)):
            res[f"{_short(name)}.{k}"] = v.detach()
        pre = xhat + (beta / gamma).view(shape)
    return u, pre, var.detach()


def forward(W, buffers, x, drop_mask=None, training=True, dtype=torch.float64, masks=None, grad=False):
    """One call.  W: CONV_PARAMS -> tensor; buffers: BUFFERS -> tensor (left alone); x (B, 1, T, F); drop_mask (B, T, Cf) or (B*T, Cf), nonzero = kept
    (None: nothing dropped).  masks: None, or five boolean tensors (layers 1 to 4 in the device's (B, T, C, F) layout, then the BatchNorm1d's
    (B, T, Cf)): each ReLU is then u * mask.  With masks=None each ReLU is relu(u), written u * (u > 0): the same values and the same derivative
    through the same operator as the masked form, so that the oracle's own decisions given as masks reproduce it to the bit.  Returns a dict: y1..y4 (B, T, C, F); per BatchNorm "<bn>.mean / .invstd / .scale / .shift"
    (<bn> = bn1..bn4, out_bn); yabs1..4 (per-channel max |y|); abound1..4 (max_c |scale_c| yabs_c + |shift_c|); pre1..pre4 (B, T, C, F) and pre5
    (B, T, Cf); dec1..dec5, the decisions bn_i(y_i) > 0 in the layouts of pre_i; var_<bn>, the variance each BatchNorm normalises with; z, out
    (B, T, Cf); "buffers": the buffers after the call (training: running_mean, running_var with the unbiased variance and momentum 0.1, num_batches_tracked + 1; eval: the buffers as they are).  With grad=True the tensors
    keep their graph and "leaves" holds the parameters `gradients` differentiates with respect to."""
    fn = torch.nn.functional
    P = {k: W[k].detach().to(dtype).clone().requires_grad_(grad) for k in CONV_PARAMS}
    res, new_buffers = {}, {k: v.clone() for k, v in buffers.items()}
    a = x.detach().to(dtype)
    Bn, _, T, F = a.shape
    for i in LAYERS:
        y = fn.conv2d(a, P[f"convstack.conv{i}.weight"], padding=1)                               # (B, C, T, F)
        u, pre, var = _bn(res, new_buffers, y, P, buffers, f"convstack.bn{i}", (0, 2, 3), (1, -1, 1, 1), training, dtype)
        a = u * ((u.detach() > 0) if masks is None else masks[i - 1].permute(0, 2, 1, 3)).to(dtype)
        with torch.no_grad():
            res[f"y{i}"], res[f"pre{i}"], res[f"var_bn{i}"] = y.detach().permute(0, 2, 1, 3).contiguous(), pre.permute(0, 2, 1, 3).contiguous(), var
            res[f"dec{i}"] = (u.detach() > 0).permute(0, 2, 1, 3).contiguous()
            res[f"yabs{i}"] = y.detach().abs().amax(dim=(0, 2, 3))
            res[f"abound{i}"] = (res[f"bn{i}.scale"].abs() * res[f"yabs{i}"] + res[f"bn{i}.shift"].abs()).max()
    z = a.transpose(1, 2).flatten(2) @ P["convstack.out.weight"].t()                              # (B, T, Cf); column k of the operand is channel k // F
    Cf = z.shape[2]
    u, pre, var = _bn(res, new_buffers, z.reshape(Bn * T, Cf), P, buffers, "convstack.out_bn", (0,), (1, -1), training, dtype)
    r = u * ((u.detach() > 0) if masks is None else masks[4].reshape(Bn * T, Cf)).to(dtype)
    if drop_mask is not None:
        r = r * ((drop_mask.reshape(Bn * T, Cf) != 0).to(dtype) / KEEP)
    out = r.view(Bn, T, Cf)
    res["dec5"] = (u.detach() > 0).view(Bn, T, Cf)
    res.update(z=z if grad else z.detach(), out=out if grad else out.detach(), pre5=pre.view(Bn, T, Cf), var_out_bn=var, buffers=new_buffers)
    if grad:
        res["leaves"] = P
    return res


def decisions(fwd):
    """The five ReLU decisions a forward took itself, bn_i(y_i) > 0, in the layout `forward` takes as masks."""
    return [fwd[f"dec{i}"] for i in (1, 2, 3, 4, 5)]


def masks_from_saved(ys, bns, z, out_bn):
    """The decisions the DEVICE took, recomputed from its own saved fp32 tensors in float64: double(y) double(scale) + double(shift) > 0.  The product
    of two fp32 numbers is exact in float64 and the sum keeps its sign, so this is the sign a single fp32 fma gives.  Also returns, per layer, the
    number of elements at which the two-rounding form fl(fl(y scale) + shift) > 0 decides otherwise (a kernel that did NOT contract the expression
    would be ambiguous there).  ys: y1..y4 (B, T, C, F); bns: their (mean, invstd, scale, shift); z (rows, Cf) or (B, T, Cf); out_bn likewise."""
    masks, ambiguous = [], []
    for t, bn, shape in [(y, bn, (1, 1, -1, 1)) for y, bn in zip(ys, bns)] + [(z, out_bn, (1,) * (z.dim() - 1) + (-1,))]:
        t, sc, sh = t.detach().cpu().float(), bn[2].detach().cpu().float().view(shape), bn[3].detach().cpu().float().view(shape)
        m = t.double() * sc.double() + sh.double() > 0
        two = (t * sc) + sh > 0                                              # (CPU torch: two fp32 roundings)
        masks.append(m)
        ambiguous.append(int((m != two).sum()))
    return masks, ambiguous


def gradients(W, buffers, x, drop_mask, training, d_out, masks=None, dtype=torch.float64):
    """The 15 gradients of CONV_PARAMS under d_out (B, T, Cf) on `out`, by torch autograd in `dtype`; masks as in `forward`."""
    f = forward(W, buffers, x, drop_mask, training, dtype, masks=masks, grad=True)
    f["out"].backward(d_out.detach().to(dtype).view_as(f["out"]))
    return {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in f["leaves"].items()}


FWD_TENSORS = tuple(f"y{i}" for i in LAYERS) + tuple(f"{_short(n)}.{k}" for n in BN_NAMES for k in BN_PARTS) + ("z", "out")
FLOAT_BUFFERS = tuple(b for b in BUFFERS if not b.endswith("num_batches_tracked"))


def forward_views(ref, got):
    """(name, ref, got) of every forward tensor: y1..y4 (B, T, C, F), the 5 x 4 BatchNorm vectors, z and out (B, T, Cf)."""
    return [(k, ref[k], got[k].view_as(ref[k])) for k in FWD_TENSORS]


def buffer_views(ref, got):
    """(name, ref, got) of the ten running statistics (num_batches_tracked is compared exactly, by the caller)."""
    return [(k, ref["buffers"][k], got[k]) for k in FLOAT_BUFFERS]


def grad_views(ref, got):
    return [(k, ref[k], got[k]) for k in CONV_PARAMS]


def reference(W, buffers, x, drop_mask, training, d_out=None):
    """The float64 run and what the float32 run of the same code loses against it: returns (f64 forward, f64 gradients or None, f32 forward, dev32).
    dev32[name] = max |f32 - f64| / max |f64| per tensor of FWD_TENSORS, per running statistic and (with d_out) per gradient; dev32["pre<i>"] is
    ABSOLUTE, max |pre32 - pre64|: the normalised pre-activation is already in units of the channel's standard deviation, and that is the unit of
    the flip margin.  The float32 gradients are taken under the float64 run's ReLU decisions, so that their deviation is rounding alone and never
    a flipped element (which moves a gradient by parts in a thousand and would widen the bar built on it)."""
    f64 = forward(W, buffers, x, drop_mask, training, torch.float64)
    f32 = forward(W, buffers, x, drop_mask, training, torch.float32)
    dev = {name: rel_err(b, a) for name, a, b in forward_views(f64, f32)}
    dev.update({name: rel_err(b, a) for name, a, b in buffer_views(f64, f32["buffers"])})
    dev.update({f"pre{i}": float((f32[f"pre{i}"].double() - f64[f"pre{i}"]).abs().max()) for i in (1, 2, 3, 4, 5)})
    g64 = None
    if d_out is not None:
        g64 = gradients(W, buffers, x, drop_mask, training, d_out)
        g32 = gradients(W, buffers, x, drop_mask, training, d_out, masks=decisions(f64), dtype=torch.float32)
        dev.update({name: rel_err(b, a) for name, a, b in grad_views(g64, g32)})
    return f64, g64, f32, dev


def rel_err(got, ref, scale=None):
    """max |got - ref| over max |ref| (or over `scale`, where the tensor compared holds more than the reference: a pre-filled gradient)."""
    d = (got.double() - ref.double()).abs()
    m = float(ref.double().abs().max()) if scale is None else float(scale)
    return float(d.max()) / max(m, 1e-300) if d.numel() else 0.0


def worst(got, ref):
    """Index (as a tuple) and size of the largest |got - ref| (a NaN counts as the largest)."""
    d = torch.nan_to_num((got.double() - ref.double()).abs(), nan=float("inf"))
    return unravel(int(d.argmax()), d.shape), float(d.max())


def unravel(i, shape):
    idx = []
    for s in reversed(shape):
        idx.append(i % s)
        i //= s
    return tuple(reversed(idx))


def where(name, at, F=None):
    """An index in words: (clip, frame, channel, bin) for the (B, T, C, F) tensors, (clip, frame, channel) for z / out / pre5."""
    if len(at) == 4 and name.startswith(("y", "pre", "layer")):
        return f"clip {at[0]}, frame {at[1]}, channel {at[2]}, bin {at[3]}"
    if len(at) == 3:
        return f"clip {at[0]}, frame {at[1]}, channel {at[2]}"
    if len(at) == 4:
        return f"output channel {at[0]}, input channel {at[1]}, tap ({at[2]}, {at[3]})"
    if len(at) == 2 and F:
        return f"feature {at[0]}, channel {at[1] // F}, bin {at[1] % F}"
    return f"channel {at[0]}" if len(at) == 1 else f"index {at}"
