"""The domain in which the key-image attention is right, and the guard that keeps a decode inside it.  Pure host code: torch ops on whatever
device the tensors live on, no kernel of its own (CPU-tested in tests/test_attn_range_cpu.py).

Every attention kernel forms  tanh(k + q) = 1 - 2 / (1 + E_K E_q)  from the key image E_K = exp(2 k) (the key projection's GEMM epilogue, act 3) and
E_q = exp(2 q) (once per row and step).  Both factors go through exp2x_clamped (csrc/a2s_common.h), which clamps ITS OWN argument to +-CLAMP whatever
the other one is.  With k~, q~ the clamped values the kernels therefore compute tanh(k~ + q~), and

    D = (|k| <= CLAMP and |q| <= CLAMP)  or  min(|k|, |q|) <= ONE_SIDED

is where that equals tanh(k + q) to within 1 - tanh(9) = 3.05e-8 (float64, a grid of 1/4 over [-70, 70]^2).  Outside D it is silently wrong by up to
1.0:  k = 50, q = -45  gives tanh(43 - 43) = 0 where tanh(5) = 0.9999."""
import warnings

import torch

# exp2x_clamped's bound: exp(+-86) is finite and normal in fp32 (2.2e37, 4.5e-38), exp(2 * 44.4) is not
CLAMP = 43.0
# One side beyond the clamp is harmless while the other is at most CLAMP - 9: the clamped side then still leaves |k~ + q~| >= 43 - 34 = 9 with the sign
# of k + q, and |k + q| >= 9 as well, so both tanh are within 1 - tanh(9) = 3.05e-8 of the same +-1 (fp32's half ulp at 1 is 2.98e-8).
ONE_SIDED = CLAMP - 9.0

# What a decode outside D does: "raise" (default) -> hip.A2SError;  "warn" -> one warnings.warn per process, the outputs are returned as computed
# (set piano_a2s_amd.attn_range.on_violation = "warn")
on_violation = "raise"
_warned = False


def in_domain(k_abs, q_abs):
    """k_abs, q_abs: the largest |k| and |q| of a launch (or bounds on them) -> whether every (k, q) pair of it lies in D."""
    k_abs, q_abs = float(k_abs), float(q_abs)
    if not (k_abs == k_abs and q_abs == q_abs):          # NaN: nothing is known
        return False
    return (k_abs <= CLAMP and q_abs <= CLAMP) or min(k_abs, q_abs) <= ONE_SIDED


def query_bound(attn_weight, attn_bias, H):
    """max_j (sum |W[j, :2H]| + |b_j|) as a 0-dim tensor on the weights' device: a bound on |q|, q = W[:, :2H] h + b, because the decoder states h are
    GRU states in (-1, 1).  attn_weight: (H, 4H), the attention Linear (query half first); attn_bias: (H,)."""
    return (attn_weight[:, :2 * H].abs().sum(dim=1) + attn_bias.abs()).max()


def key_range(image):
    """The largest |k| the key image exp(2 k) holds, 0.5 * max(|ln min|, |ln max|), as a 0-dim tensor on the image's device.  The image saturates at
    exp(+-2 CLAMP), so a reading of CLAMP means "CLAMP or more"; the static L1 bound on the key half is far too loose to decide anything (the
    procedural weights at hidden size 256 already exceed it), which is why the keys are measured and only the queries are bounded."""
    lo, hi = torch.aminmax(image)
    return 0.5 * torch.maximum(lo.log().abs(), hi.log().abs())


def violations(layers, k_abs, q_abs):
    """layers: names; k_abs, q_abs: their readings (host numbers) -> [(name, k, q)] of the layers outside D."""
    return [(n, float(k), float(q)) for n, k, q in zip(layers, k_abs, q_abs) if not in_domain(k, q)]


def message(bad):
    return "; ".join(f"{n}: max |k| = {k:.4g}{' (saturated: this or more)' if k >= CLAMP - 1e-3 else ''}, bound on |q| = {q:.4g}" for n, k, q in bad) + \
        f" -- the key-image attention equals tanh(k + q) only while both are <= {CLAMP:g} or one of them is <= {ONE_SIDED:g} (include/a2s.h)"


def report(bad, error):
    """bad: violations(...); error: the exception class to raise.  Raises, or warns once per process (on_violation)."""
    global _warned
    if not bad:
        return
    if on_violation == "raise":
        raise error("attention pre-activations outside the key image's domain: " + message(bad))
    if on_violation != "warn":
        raise ValueError(f"attn_range.on_violation must be 'raise' or 'warn' (got {on_violation!r})")
    if not _warned:
        _warned = True
        warnings.warn("attention pre-activations outside the key image's domain, the outputs are not those of tanh(k + q): " + message(bad), RuntimeWarning,
                      stacklevel=3)
