"""TEST INFRASTRUCTURE ONLY.  One encoder call (Engine.encoder / engine_bwd._encoder_bwd: two bidirectional GRU layers and the fc/tanh bridge)
restated in plain torch on the CPU, in float64 or float32: what tests/test_gpu_encoder_call.py holds every path of the call to, tensor by tensor.

Built on oracle/model_ref.py's `gru_direction` (and checked against its `encoder_forward`), shaped like tests/note_decoder_oracle.py.  What the call
exposes beyond model_ref.encoder_forward:
  * gi = x W_ih^T + b_ih of every layer and direction is a tensor of its own.  gru_direction is fed gi in the place of the features and the
    identity in the place of W_ih (zero b_ih): gi I^T + 0 = gi exactly (products with 1 and 0, sums with 0), in either precision; autograd then
    leaves the gradient with respect to gi -- the `dgi_all` of a2s_gru_seq_bwd -- in gi.grad, so that a failure can be placed before or after the
    deferred products (dX, dW_ih, db_ih are products of dgi);
  * the gates in the library's saved layout (T, B, 4H) = [r | z | n | W_hn h + b_hn], by gru_cell's formulas from gi and the outputs;
  * the four final states (order l0, l0_reverse, l1, l1_reverse) and hidden = [tanh(fc([hf0; hr0])) | tanh(fc([hf1; hr1]))].

Imports nothing of the product package."""
import torch

from oracle.model_ref import gru_direction

SUFFIXES = ("l0", "l0_reverse", "l1", "l1_reverse")
GRU_PARAMS = tuple(f"encoder.gru.{k}_{s}" for s in SUFFIXES for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
PARAMS = GRU_PARAMS + ("encoder.fc.weight", "encoder.fc.bias")          # the 18 tensors of the encoder, by the reference's state_dict names


def encoder_tensors(state):
    """The 18 encoder tensors out of a state dict."""
    return {k: state[k] for k in PARAMS}


def gates_of(gi, out, w_hh, b_hh, reverse):
    """(T, B, 4H) = [r | z | n | gh_n] of one direction from gi (B, T, 3H) and its outputs (B, T, H): h_prev of frame t is the output of the frame
    processed before it (zero at the first processed frame)."""
    H = out.shape[2]
    zero = torch.zeros_like(out[:, :1])
    hprev = torch.cat([out[:, 1:], zero], dim=1) if reverse else torch.cat([zero, out[:, :-1]], dim=1)
    gh = hprev @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return torch.cat([r, z, n, gh[..., 2 * H:]], dim=2).transpose(0, 1).contiguous(), hprev


def encoder_call(W, x, dtype=torch.float64, grad=False):
    """One call.  W: PARAMS -> tensor; x (B, T, I) features.  Returns a dict: gi_<sfx> (B, T, 3H), out_l0 / out_l1 (B, T, 2H) = [forward | reverse],
    gates_<sfx> (T, B, 4H), hn_<sfx> (B, H), hidden (B, 2H).  With grad=True the tensors keep their graph and `leaves` holds what `call_backward`
    differentiates with respect to."""
    P = {k: W[k].detach().to(dtype).clone().requires_grad_(grad) for k in PARAMS}
    x_l = x.detach().to(dtype).clone().requires_grad_(grad)
    H = P["encoder.gru.weight_hh_l0"].shape[1]
    eye, zero = torch.eye(3 * H, dtype=dtype), torch.zeros(3 * H, dtype=dtype)
    res, gis, finals = {}, {}, []
    inp = x_l
    for layer in (0, 1):
        outs = []
        for d, sfx in enumerate((f"l{layer}", f"l{layer}_reverse")):
            w_hh, b_hh = P[f"encoder.gru.weight_hh_{sfx}"], P[f"encoder.gru.bias_hh_{sfx}"]
            gi = inp @ P[f"encoder.gru.weight_ih_{sfx}"].t() + P[f"encoder.gru.bias_ih_{sfx}"]
            if grad:
                gi.retain_grad()
            Q = {"g.weight_ih_d": eye, "g.bias_ih_d": zero, "g.weight_hh_d": w_hh, "g.bias_hh_d": b_hh}
            out, hn = gru_direction(gi, Q, "g", "d", reverse=d == 1)
            with torch.no_grad():
                res[f"gates_{sfx}"], _ = gates_of(gi.detach(), out.detach(), w_hh.detach(), b_hh.detach(), d == 1)
            gis[sfx], res[f"gi_{sfx}"], res[f"hn_{sfx}"] = gi, gi, hn
            outs.append(out)
            finals.append(hn)
        inp = res[f"out_l{layer}"] = torch.cat(outs, dim=2)
    fc_w, fc_b = P["encoder.fc.weight"], P["encoder.fc.bias"]
    res["hidden"] = torch.cat([torch.tanh(torch.cat([finals[2 * l], finals[2 * l + 1]], dim=1) @ fc_w.t() + fc_b) for l in (0, 1)], dim=1)
    res["leaves"] = dict(P=P, x=x_l, gi=gis)
    return res


def call_backward(fwd, dEnc, d_hidden):
    """Reverse of encoder_call(grad=True) under dEnc (B, T, 2H) on layer 1's outputs and d_hidden (B, 2H).  Returns dict(dX (B, T, I), dgi_<sfx>
    (B, T, 3H), params: PARAMS -> gradient)."""
    dt = fwd["hidden"].dtype
    lv = fwd["leaves"]
    for t in [lv["x"], *lv["P"].values(), *lv["gi"].values()]:
        t.grad = None
    torch.autograd.backward([fwd["out_l1"], fwd["hidden"]], [dEnc.detach().to(dt), d_hidden.detach().to(dt)])
    zero = lambda t: t.grad.detach() if t.grad is not None else torch.zeros_like(t)
    g = {"dX": zero(lv["x"]), "params": {k: zero(v) for k, v in lv["P"].items()}}
    g.update({f"dgi_{s}": zero(t) for s, t in lv["gi"].items()})
    return g


FWD_TENSORS = tuple(f"gi_{s}" for s in SUFFIXES) + ("out_l0", "out_l1") + tuple(f"gates_{s}" for s in SUFFIXES) + tuple(f"hn_{s}" for s in SUFFIXES) + ("hidden",)


def forward_views(ref, got):
    """(name, ref, got) of every forward tensor, clip first: (B, T, width) -- the saved gates transposed to it -- or (B, width)."""
    bt = lambda k, t: t.transpose(0, 1) if k.startswith("gates_") else t
    return [(k, bt(k, ref[k]), bt(k, got[k])) for k in FWD_TENSORS]


def grad_views(ref, got, dgi=False):
    out = [("dX", ref["dX"], got["dX"])] + [(k, ref["params"][k], got["params"][k]) for k in PARAMS]
    return out + ([(f"dgi_{s}", ref[f"dgi_{s}"], got[f"dgi_{s}"]) for s in SUFFIXES] if dgi else [])


def reference(W, x, dEnc=None, d_hidden=None):
    """The float64 run and what the float32 run of the same code loses against it: returns (f64 forward dict, f64 gradients or None, f32 forward dict,
    dev32) with dev32[name] = max |f32 - f64| / max |f64| per tensor of FWD_TENSORS and, with dEnc / d_hidden, per gradient of grad_views(dgi=True)."""
    runs = {}
    for dt in (torch.float64, torch.float32):
        f = encoder_call(W, x, dtype=dt, grad=dEnc is not None)
        g = call_backward(f, dEnc, d_hidden) if dEnc is not None else None
        runs[dt] = ({k: v.detach() for k, v in f.items() if k != "leaves"}, g)
    (f64, g64), (f32, g32) = runs[torch.float64], runs[torch.float32]
    dev = {name: rel_err(b, a) for name, a, b in forward_views(f64, f32)}
    if g64 is not None:
        dev.update({name: rel_err(b, a) for name, a, b in grad_views(g64, g32, dgi=True)})
    return f64, g64, f32, dev


def rel_err(got, ref, scale=None):
    """max |got - ref| over max |ref| (or over `scale`, where the tensor compared holds more than the reference: a pre-filled gradient)."""
    d = (got.double() - ref.double()).abs()
    m = float(ref.double().abs().max()) if scale is None else float(scale)
    return float(d.max()) / max(m, 1e-300) if d.numel() else 0.0


def worst(got, ref):
    """Index (as a tuple) and size of the largest |got - ref| (a NaN counts as the largest): tells the author WHICH clip, frame and column are wrong."""
    d = torch.nan_to_num((got.double() - ref.double()).abs(), nan=float("inf"))
    i = int(d.argmax())
    idx = []
    for s in reversed(d.shape):
        idx.append(i % s)
        i //= s
    return tuple(reversed(idx)), float(d.max())


def where(name, at):
    """The index `worst` found, in words: clip, frame and column for the (B, T, width) tensors, clip and column for the (B, width) ones."""
    if name.startswith(("gi_", "out_", "gates_", "dgi_")) or name == "dX":
        return f"clip {at[0]}, frame {at[1]}, column {at[2]}"
    if name.startswith("hn_") or name == "hidden":
        return f"clip {at[0]}, column {at[1]}"
    return f"index {at}"
