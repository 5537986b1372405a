"""tests/convstack_oracle.py checked on the CPU -- against oracle/model_ref.convstack_forward, test_gpu_operand_ranges.ref_convstack under autograd and
torch.nn.BatchNorm{1,2}d -- and the preconditions of every input tests/test_gpu_convstack_call.py runs, asserted over the tables that file uses.

The preconditions (per input and per ReLU layer 1..5, the fifth being the BatchNorm1d's):
  (a) FLIP_MARGIN = max(7e-6, 3 x the deviation of the float32 oracle's normalised pre-activation from the float64 one), in standard deviations of
      the channel (test_gpu_convstack_call.flip_margins);
  (b) at most 1e-4 of a layer's float64 pre-activations lie within FLIP_MARGIN of the threshold (a Gaussian density gives about 6e-6): the elements
      whose decision the device may take either way are few, and the count per input and layer is reported;
  (c) every decision in which the float32 oracle differs from the float64 one lies within FLIP_MARGIN: the margin covers what float32 arithmetic of
      this chain does to a decision;
  (d) B * T >= 2 and a positive variance in every BatchNorm channel.  rows = 1 in training mode is undefined in torch (nn.BatchNorm1d raises) and is
      left out of the cases."""
import pytest
import torch

from tests import convstack_oracle as oracle
from tests import test_gpu_convstack_call as call
from tests.test_gpu_operand_ranges import CONV_PARAMS, _report, ref_convstack


def _tiny(seed=3, F=8, Cf=12, B=2, T=5, dtype=torch.float64):
    from piano_a2s_amd import spec
    cfg = spec.default_cfg(freq_bins=F, conv_feature_size=Cf)
    W, buffers = oracle.convstack_tensors(spec.procedural_state(cfg, seed))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, F, generator=g, dtype=dtype)
    d_out = torch.randn(B, T, Cf, generator=g, dtype=dtype)
    return {k: v.to(dtype) for k, v in W.items()}, {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in buffers.items()}, x, d_out


def test_parameter_list_is_the_chain_tests():
    assert list(oracle.CONV_PARAMS) == list(CONV_PARAMS)


@pytest.mark.parametrize("training", [True, False])
def test_forward_equals_model_ref(training):
    from oracle import model_ref
    W, buffers, x, _ = _tiny()
    got = oracle.forward(W, buffers, x, None, training)
    Bf = {k: v.clone() for k, v in buffers.items()}
    with torch.no_grad():
        ref = model_ref.convstack_forward(x, W, Bf, training, dropout=False)
    assert float((got["out"] - ref).abs().max()) < 1e-10
    for k in oracle.BUFFERS:                                    # model_ref updates its buffers in place; the oracle returns them and leaves its input alone
        assert float((got["buffers"][k].double() - Bf[k].double()).abs().max()) < 1e-10, k
        if not training:
            assert torch.equal(got["buffers"][k], buffers[k]), k
    assert int(got["buffers"]["convstack.bn1.num_batches_tracked"]) == int(buffers["convstack.bn1.num_batches_tracked"]) + int(training)


def test_saved_tensors_are_what_they_are_called():
    """scale / shift reproduce bn(y) from y; pre is bn(y) / gamma; yabs and abound are the formulas of the module docstring; dec is bn(y) > 0."""
    W, buffers, x, _ = _tiny()
    f = oracle.forward(W, buffers, x, None, True)
    for i in oracle.LAYERS:
        sc, sh, gamma = (t.view(1, 1, -1, 1) for t in (f[f"bn{i}.scale"], f[f"bn{i}.shift"], W[f"convstack.bn{i}.weight"]))
        u = f[f"y{i}"] * sc + sh
        assert float((u / gamma - f[f"pre{i}"]).abs().max()) < 1e-10
        assert torch.equal(f[f"dec{i}"] | (u.abs() < 1e-10), (u > 0) | (u.abs() < 1e-10))
        assert torch.equal(f[f"yabs{i}"], f[f"y{i}"].abs().amax(dim=(0, 1, 3)))
        assert float(f[f"abound{i}"]) >= float(torch.relu(u).max())
        assert float((f[f"bn{i}.invstd"] - 1 / torch.sqrt(f[f"y{i}"].var(dim=(0, 1, 3), unbiased=False) + 1e-5)).abs().max()) < 1e-10
    u5 = f["z"] * f["out_bn.scale"] + f["out_bn.shift"]
    assert float((torch.relu(u5) - f["out"]).abs().max()) < 1e-10


def test_gradients_equal_the_chain_tests_reference_under_autograd():
    W, buffers, x, d_out = _tiny()
    got = oracle.gradients(W, buffers, x, None, True, d_out)
    P = {k: W[k].clone().requires_grad_(True) for k in CONV_PARAMS}
    out, _ = ref_convstack(x, P)
    out.backward(d_out)
    for k in CONV_PARAMS:
        assert oracle.rel_err(got[k], P[k].grad) < 1e-10, k


def test_own_decisions_as_masks_reproduce_the_relu_exactly():
    W, buffers, x, d_out = _tiny()
    g = torch.Generator().manual_seed(5)
    drop = (torch.rand(x.shape[0] * x.shape[2], 12, generator=g) >= 0.2).to(torch.uint8)
    f = oracle.forward(W, buffers, x, drop, True)
    plain = oracle.gradients(W, buffers, x, drop, True, d_out)
    masked = oracle.gradients(W, buffers, x, drop, True, d_out, masks=oracle.decisions(f))
    for k in CONV_PARAMS:
        assert torch.equal(plain[k], masked[k]), k
    fm = oracle.forward(W, buffers, x, drop, True, masks=oracle.decisions(f))
    assert torch.equal(fm["out"], f["out"]) and torch.equal(fm["z"], f["z"])
    share = float((f["out"].reshape(-1, 12)[drop == 0] == 0).float().mean())
    assert share == 1.0 and 0.1 < 1 - float(drop.float().mean()) < 0.3


def test_running_statistics_equal_torch_batchnorm_over_three_calls():
    W, buffers, x, _ = _tiny()
    nn = torch.nn
    mods = [nn.BatchNorm2d(20), nn.BatchNorm2d(20), nn.BatchNorm2d(40), nn.BatchNorm2d(40), nn.BatchNorm1d(12)]
    for m, name in zip(mods, oracle.BN_NAMES):
        m.double()
        m.load_state_dict({k: (W if k in ("weight", "bias") else buffers)[f"{name}.{k}"].clone() for k in ("weight", "bias", "running_mean", "running_var",
                                                                                                         "num_batches_tracked")})
        m.train()
    g = torch.Generator().manual_seed(8)
    fn = torch.nn.functional
    for call_no in range(3):
        xin = torch.randn(x.shape, generator=g, dtype=torch.float64)
        f = oracle.forward(W, buffers, xin, None, True)
        a = xin
        with torch.no_grad():
            for i in oracle.LAYERS:
                a = torch.relu(mods[i - 1](fn.conv2d(a, W[f"convstack.conv{i}.weight"], padding=1)))
            z = a.transpose(1, 2).flatten(2) @ W["convstack.out.weight"].t()
            out = torch.relu(mods[4](z.reshape(-1, 12))).view_as(f["out"])
        assert float((out - f["out"]).abs().max()) < 1e-10
        buffers = f["buffers"]
        for m, name in zip(mods, oracle.BN_NAMES):
            for k in ("running_mean", "running_var"):
                assert float((getattr(m, k) - buffers[f"{name}.{k}"]).abs().max()) < 1e-12, (call_no, name, k)
            assert int(m.num_batches_tracked) == int(buffers[f"{name}.num_batches_tracked"]) == 3 + call_no + 1          # (procedural_state starts them at 3)


def test_one_flipped_decision_moves_a_gradient_beyond_its_bar():
    """The comparison can see a flip: with ONE decision of layer 2 inverted at least one gradient leaves max(2e-5, 3 x float32 deviation) of the
    unflipped ones -- for the element of the largest |bn(y)| (the activation itself changes) and for the element nearest the threshold (the
    activation hardly changes, but its gradient passes or does not: the discontinuity that makes the GPU test take the device's decisions)."""
    B, T, F = call.SMALL
    i = call.inputs(B, T, F)
    f64, g64, _, dev32 = call.reference(B, T, F)
    for pick in ("far", "near"):
        masks = [m.clone() for m in oracle.decisions(f64)]
        pre = f64["pre2"].abs()
        at = oracle.unravel(int(pre.argmax() if pick == "far" else pre.argmin()), pre.shape)
        masks[1][at] = ~masks[1][at]
        g = oracle.gradients(i["W"], i["buffers"], i["x"], None, True, i["d_out"], masks=masks)
        ratios = {k: oracle.rel_err(g[k], g64[k]) / max(call.GRAD_BAR, 3 * dev32[k]) for k in CONV_PARAMS}
        worst = max(ratios, key=ratios.get)
        _report(f"convstack oracle: one layer-2 decision flipped {pick} from the threshold (|pre| {float(pre[at]):.3e}), worst gradient error / bar ({worst})", ratios[worst])
        print(pick, float(pre[at]), worst, ratios[worst])
        assert ratios[worst] > 1.0, (pick, worst, ratios[worst])


def test_masks_from_saved_is_the_fma_sign():
    """Built cases: y scale + shift that an fma puts on one side and two roundings on the other (or on zero) -- the float64 evaluation follows the fma."""
    y = torch.tensor([1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23, 3.0]).view(1, 1, 3, 1)
    scale = torch.tensor([1.0 + 2.0 ** -23, 1.0, -1.0])
    shift = torch.tensor([-(1.0 + 2.0 ** -22), -1.0, 3.0])          # channel 0: the exact product exceeds -shift by 2^-46, its fp32 rounding equals it
    bn = (None, None, scale, shift)
    z, out_bn = torch.zeros(2, 3), (None, None, torch.ones(3), torch.zeros(3))
    masks, ambiguous = oracle.masks_from_saved([y], [bn], z, out_bn)
    assert masks[0].flatten().tolist() == [True, True, False] and ambiguous == [1, 0]
    assert not bool(masks[1].any())


INPUT_IDS = [f"B{c[0]}_T{c[1]}_F{c[2]}-{v}" for c, v in call.INPUTS]


def test_the_tables_cover_what_the_gpu_tests_run():
    assert set(call.PATH_CASES) <= set(call.CASES) and call.BIG in call.CASES and call.SMALL in call.CASES
    assert set(call.FACTS) == set(call.CASES)
    assert {c for c, _ in call.INPUTS} == set(call.CASES)


@pytest.mark.parametrize("case,variant", call.INPUTS, ids=INPUT_IDS)
def test_preconditions_of_the_gpu_inputs(case, variant):
    B, T, F = case
    f64, _, f32, dev32 = call.reference(B, T, F, variant)
    margins = call.flip_margins(dev32)                                                   # (a)
    label = f"convstack_call preconditions B{B}_T{T}_F{F}-{variant}"
    assert B * T >= 2                                                                    # (d)
    for name in oracle.BN_NAMES:
        assert float(f64["var_" + name[len("convstack."):]].min()) > 0.0, name
    for i, margin in enumerate(margins, start=1):
        assert margin >= call.CHAIN_MARGIN and margin >= 3 * dev32[f"pre{i}"]
        pre = f64[f"pre{i}"]
        near = int((pre.abs() <= margin).sum())                                          # (b)
        _report(f"{label}: layer {i} margin {margin:.3e}, float64 pre-activations within it (of {pre.numel()})", float(near))
        print(f"{label}: layer {i} margin {margin:.3e} (float32 deviation {dev32[f'pre{i}']:.3e}); {near} of {pre.numel()} within it")
        assert near <= call.NEAR_SHARE * pre.numel(), (i, near, pre.numel())
        differ = f32[f"dec{i}"] != f64[f"dec{i}"]                                        # (c)
        assert not bool((differ & (pre.abs() > margin)).any()), (i, int(differ.sum()), float(pre.abs()[differ].max()))
        assert call.flips(f64, oracle.decisions(f32), margins)[i - 1] == (int(differ.sum()), None)
