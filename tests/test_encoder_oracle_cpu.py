"""tests/encoder_oracle.py proved without a GPU: against torch.nn.GRU(num_layers=2, bidirectional=True) in float64 loaded with the same tensors
(outputs, h_n, every GRU parameter gradient) at a small width and at 256, against oracle/model_ref.py's encoder_forward, and in itself (the saved
gates rebuild the outputs, the gi gradients rebuild dX, dW_ih and db_ih); then the preconditions of the inputs tests/test_gpu_encoder_call.py runs."""
import pytest
import torch

from oracle import model_ref
from tests import encoder_oracle as oracle
from tests import test_gpu_encoder_call as call


def _random_encoder(H, I, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1)
    W = {}
    for n, sfx in enumerate(oracle.SUFFIXES):
        In = I if n < 2 else 2 * H
        W[f"encoder.gru.weight_ih_{sfx}"] = r(3 * H, In) * (3.0 / In) ** 0.5
        W[f"encoder.gru.weight_hh_{sfx}"] = r(3 * H, H) * (3.0 / H) ** 0.5
        W[f"encoder.gru.bias_ih_{sfx}"], W[f"encoder.gru.bias_hh_{sfx}"] = r(3 * H) * 0.1, r(3 * H) * 0.1
    W["encoder.fc.weight"], W["encoder.fc.bias"] = r(H, 2 * H) * (1.5 / H) ** 0.5, r(H) * 0.1
    return W, g


@pytest.mark.parametrize("H,I,B,T", [(8, 6, 3, 7), (256, 256, 2, 5)])
def test_oracle_equals_torch_gru(H, I, B, T):
    W, g = _random_encoder(H, I, 5 + H)
    x = torch.relu(torch.randn(B, T, I, generator=g, dtype=torch.float64))
    dEnc, d_hidden = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64), torch.randn(B, 2 * H, generator=g, dtype=torch.float64)
    f = oracle.encoder_call(W, x, grad=True)
    gr = oracle.call_backward(f, dEnc, d_hidden)
    # ---- torch.nn.GRU with the same tensors; the bridge by its definition, so that h_n receives the same gradient
    gru = torch.nn.GRU(I, H, num_layers=2, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for k in oracle.GRU_PARAMS:
            getattr(gru, k[len("encoder.gru."):]).copy_(W[k])
    xt = x.clone().requires_grad_(True)
    fc_w, fc_b = W["encoder.fc.weight"].clone().requires_grad_(True), W["encoder.fc.bias"].clone().requires_grad_(True)
    out, hn = gru(xt)                                       # hn (4, B, H): l0, l0_reverse, l1, l1_reverse
    hidden = torch.cat([torch.tanh(torch.cat([hn[2 * l], hn[2 * l + 1]], dim=1) @ fc_w.t() + fc_b) for l in (0, 1)], dim=1)
    torch.autograd.backward([out, hidden], [dEnc, d_hidden])
    tol = dict(rtol=0, atol=1e-12)
    assert torch.allclose(f["out_l1"], out, **tol) and torch.allclose(f["hidden"], hidden, **tol)
    for n, sfx in enumerate(oracle.SUFFIXES):
        assert torch.allclose(f[f"hn_{sfx}"], hn[n], **tol), sfx
    assert oracle.rel_err(gr["dX"], xt.grad) < 1e-12
    for k in oracle.GRU_PARAMS:
        assert oracle.rel_err(gr["params"][k], getattr(gru, k[len("encoder.gru."):]).grad) < 1e-12, k
    assert oracle.rel_err(gr["params"]["encoder.fc.weight"], fc_w.grad) < 1e-12 and oracle.rel_err(gr["params"]["encoder.fc.bias"], fc_b.grad) < 1e-12
    # ---- model_ref.encoder_forward (what the whole-model oracle runs)
    enc_ref, hid_ref = model_ref.encoder_forward(x, W)
    assert torch.allclose(f["out_l1"], enc_ref, **tol) and torch.allclose(f["hidden"], hid_ref[0], **tol)
    # ---- the call's own tensors
    for n, sfx in enumerate(oracle.SUFFIXES):
        layer, d = n // 2, n % 2
        inp = x if layer == 0 else f["out_l0"].detach()
        gi, gates = f[f"gi_{sfx}"].detach(), f[f"gates_{sfx}"]
        assert gates.shape == (T, B, 4 * H)
        assert torch.allclose(gi, inp @ W[f"encoder.gru.weight_ih_{sfx}"].t() + W[f"encoder.gru.bias_ih_{sfx}"], **tol)
        o = f[f"out_l{layer}"].detach()[..., d * H:(d + 1) * H]
        zero = torch.zeros(B, 1, H, dtype=torch.float64)
        hprev = torch.cat([o[:, 1:], zero], 1) if d else torch.cat([zero, o[:, :-1]], 1)
        r, z, ng, ghn = [t.transpose(0, 1) for t in gates.split(H, dim=2)]
        assert torch.allclose((1 - z) * ng + z * hprev, o, **tol), f"{sfx}: the saved gates do not rebuild the outputs"
        assert torch.allclose(ghn, hprev @ W[f"encoder.gru.weight_hh_{sfx}"][2 * H:].t() + W[f"encoder.gru.bias_hh_{sfx}"][2 * H:], **tol)
        assert torch.allclose(ng, torch.tanh(gi[..., 2 * H:] + r * ghn), **tol)
        assert torch.allclose(f[f"hn_{sfx}"].detach(), o[:, 0 if d else T - 1], **tol)
        # the deferred products of the gi gradient
        dgi = gr[f"dgi_{sfx}"].reshape(B * T, 3 * H)
        assert oracle.rel_err(dgi.t() @ inp.reshape(B * T, -1), gr["params"][f"encoder.gru.weight_ih_{sfx}"]) < 1e-12
        assert oracle.rel_err(dgi.sum(0), gr["params"][f"encoder.gru.bias_ih_{sfx}"]) < 1e-12
    dX = sum(gr[f"dgi_{s}"] @ W[f"encoder.gru.weight_ih_{s}"] for s in ("l0", "l0_reverse"))
    assert oracle.rel_err(dX, gr["dX"]) < 1e-12


def test_helpers_name_the_element():
    ref = torch.zeros(3, 4, 5)
    got = ref.clone()
    got[2, 1, 3] = 0.5
    ref[0, 0, 0] = 2.0
    got[0, 0, 0] = 2.0
    assert oracle.rel_err(got, ref) == 0.25 and oracle.rel_err(got, ref, scale=0.5) == 1.0
    assert oracle.worst(got, ref) == ((2, 1, 3), 0.5)
    assert oracle.where("out_l1", (2, 1, 3)) == "clip 2, frame 1, column 3" and oracle.where("hidden", (2, 7)) == "clip 2, column 7"
    got[1, 0, 0] = float("nan")
    assert oracle.worst(got, ref)[0] == (1, 0, 0)


ALL_INPUTS = [(b, t, "plain") for b, t in call.CASES] + [(b, t, "saturated") for b, t in call.SATURATED] + [(37, 29, "small")]


@pytest.mark.parametrize("B,T,variant", ALL_INPUTS, ids=[f"B{b}_T{t}-{v}" for b, t, v in ALL_INPUTS])
def test_case_preconditions(B, T, variant):
    i = call.inputs(B, T, variant)
    x = i["x"]
    assert set(i["W"]) == set(oracle.PARAMS) and i["W"]["encoder.gru.weight_ih_l0"].shape == (3 * call.H, call.I)
    assert i["W"]["encoder.gru.weight_ih_l1"].shape == (3 * call.H, 2 * call.H)            # layer 1: I = 512, where the tall-K kernel qualifies
    assert x.shape == (B, T, call.I) and float(x.min()) == 0.0 and float(x.max()) > 0.0     # ReLU and dropout: non-negative, with exact zeros
    f64, g64, f32, dev32 = call.reference(B, T, variant)
    assert all(torch.isfinite(v).all() for v in f64.values()) and all(torch.isfinite(r).all() for _, r, _ in oracle.grad_views(g64, g64, dgi=True))
    for k in ("out_l0", "out_l1"):
        assert float(f64[k].abs().max()) <= 1.0 and float(f32[k].abs().max()) <= 1.0
    # every compared tensor is alive: an all-zero reference would make its relative error meaningless
    # (but dW_hh at T = 1: exactly zero, and the call must leave it so)
    for name, r, _ in oracle.forward_views(f64, f64) + oracle.grad_views(g64, g64):
        assert float(r.abs().max()) > 0.0 or (T == 1 and ".weight_hh_" in name), name
    if variant == "plain":
        # lively, unsaturated states: the default cases measure round-off, not clamping
        assert 0.3 < float(f64["out_l1"].abs().max()) < 0.999
        assert max(dev32.values()) < 1e-4, max(dev32.items(), key=lambda kv: kv[1])
    if variant == "saturated":
        for k in ("out_l0", "out_l1"):
            share = float((f32[k].abs() == 1.0).float().mean())
            assert share >= 0.01, f"{k}: {share:.4f} of the float32 oracle's outputs are exactly +-1.0"
    if variant == "small":
        assert float(x.max()) < 1e-2 and float(i["dEnc"].abs().max()) < 1e-5 and float(i["d_hidden"].abs().max()) < 1e-5


def test_gradient_at_one_frame_is_the_first_step_alone():
    """T = 1: h_prev = 0, so W_hh receives no gradient, b_hh the gate gradients of the only step."""
    _, g64, _, _ = call.reference(1, 1)
    for sfx in oracle.SUFFIXES:
        assert float(g64["params"][f"encoder.gru.weight_hh_{sfx}"].abs().max()) == 0.0
        assert float(g64["params"][f"encoder.gru.bias_hh_{sfx}"].abs().max()) > 0.0
