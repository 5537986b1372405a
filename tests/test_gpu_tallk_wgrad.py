"""Products over a tall reduction index on the Linear's weight-gradient kernel (csrc/a2s_linear.hip, a2s_tallk_wgrad: the encoder GRU's weight
gradients dW_ih / dW_hh with their bias sums, and the attention key products dW_e += dK^T enc) against float64 and against the generic split-K
two-term GEMM with the same operand ranges.  The measure and the bars are those of
tests/test_gpu_linear_dgrad.py::test_linear_weight_gradient_kernel: error relative to sum |a||b|, new < 1e-6, new <= 2 x generic + 1e-7, G starts
non-zero.  The Linear's own call must give the bits it gave before the kernel was generalised (tests/golden/lin_wgrad_parent_2373x384.npy)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _case(dev, M, Np, K, transposed, gscale, p_wide=False, a_wide=False, g_wide=False, with_bias=True):
    """P (M, Np) packed, A (M, K) staged; the gradient operand (scaled by gscale, one row by 2^-12) is the staged one in the transposed form
    (the encoder's use) and the packed one otherwise (the key products' use).  *_wide: the operand / the result sits at a column offset inside
    a wider tensor (P, A: offset 256 of a 512-wide tensor; G: offset 512 of a 1024-wide one)."""
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(M * 7 + Np + K + int(transposed))
    ldp, p_off = (512, 256) if p_wide else (Np, 0)
    lda, a_off = (512, 256) if a_wide else (K, 0)
    rows_g, cols_g = (K, Np) if transposed else (Np, K)
    ldg, g_off = (1024, 512) if g_wide else (cols_g, 0)
    assert p_off + Np <= ldp and a_off + K <= lda and g_off + cols_g <= ldg
    sp, sa = (1.0, gscale) if transposed else (gscale, 1.0)
    Pw = (torch.randn(M, ldp, generator=g) * sp).to(dev)
    Aw = (torch.randn(M, lda, generator=g) * sa).to(dev)
    (Aw if transposed else Pw)[M // 3] *= 2.0 ** -12
    G0 = (torch.randn(rows_g, ldg, generator=g) * gscale).to(dev)
    b0 = (torch.randn(K, generator=g) * sa).to(dev)
    pmax, amax = hip.absmax(Pw), hip.absmax(Aw)            # (of the wide tensors: a bound, and the same for both paths)
    assert L.a2s_tallk_wgrad_eligible(M, Np, K, ldp, lda, ldg, int(transposed)) == 1
    runs = []
    for _ in range(2):
        G_new, b_new = G0.clone(), b0.clone()
        n0 = L.a2s_debug_get(b"tallk_wgrad_launches")
        assert hip.tallk_wgrad(Pw, p_off, ldp, Aw, a_off, lda, G_new, g_off, ldg, M, Np, K, pmax, amax, transposed=transposed,
                               bias=b_new if with_bias else None)
        assert L.a2s_debug_get(b"tallk_wgrad_launches") == n0 + 1
        runs.append((G_new, b_new))
    G_old = G0.clone()
    if transposed:
        sk = L.a2s_gemm_pick_splitk(K, Np, M, 1)
        hip.gemm(Aw, 1, lda, Pw, ldp, 1, G_old, ldg, K, Np, M, beta=1.0, splitk=sk, a_off=a_off, b_off=p_off, c_off=g_off, two_term=(amax, pmax))
    else:
        sk = L.a2s_gemm_pick_splitk(Np, K, M, 1)
        hip.gemm(Pw, 1, ldp, Aw, lda, 1, G_old, ldg, Np, K, M, beta=1.0, splitk=sk, a_off=p_off, b_off=a_off, c_off=g_off, two_term=(pmax, amax))
    torch.cuda.synchronize()
    (G_new, b_new), (G_2, b_2) = runs
    assert torch.equal(G_new, G_2) and torch.equal(b_new, b_2), "two calls must give the same bits"
    P, A = Pw[:, p_off:p_off + Np].double(), Aw[:, a_off:a_off + K].double()
    prod, mag = P.t() @ A, P.abs().t() @ A.abs()
    if transposed:
        prod, mag = prod.t(), mag.t()
    sl = slice(g_off, g_off + cols_g)
    ref = G0[:, sl].double() + prod
    mag = G0[:, sl].double().abs() + mag
    assert torch.isfinite(G_new).all()
    err_new = float(((G_new[:, sl].double() - ref).abs() / mag.clamp_min(1e-300)).max())
    err_old = float(((G_old[:, sl].double() - ref).abs() / mag.clamp_min(1e-300)).max())
    print(f"M={M} Np={Np} K={K} transposed={transposed} gscale={gscale:g}: {err_new:.3e} of sum|p||a| (generic: {err_old:.3e})")
    assert err_new < 1e-6, f"{err_new:.3e} of sum|p||a| (generic tile: {err_old:.3e})"
    assert err_new <= 2.0 * err_old + 1e-7, f"{err_new:.3e} vs the generic tile's {err_old:.3e}"
    if g_wide:
        keep = torch.ones(ldg, dtype=torch.bool, device=dev)
        keep[sl] = False
        assert torch.equal(G_new[:, keep], G0[:, keep]), "columns of G outside the result must come back bit-identical"
    if with_bias:
        want = b0.double() + A.sum(0)
        e = float(((b_new.double() - want).abs() / A.abs().sum(0).clamp_min(1e-300)).max())
        print(f"  bias sums: {e:.3e} of sum|x| per column")
        assert e <= 1e-6, f"bias sums: {e:.3e} of sum|x| per column"
    else:
        assert torch.equal(b_new, b0)


# rows, packed columns, staged columns: one row block with the split clipped to 1; a ragged last block, three column blocks of the packed operand,
# an odd block count per split; the accumulation sign's alternation every 8 steps (4 row blocks) with several splits; two packed blocks
# against six column tiles
SHAPES = [(64, 256, 128), (327, 768, 256), (2 * 1201 + 5, 256, 512), (2 * 1201, 512, 768)]


@pytest.mark.parametrize("gscale", [1e-7, 1.0, 1e3])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("M,Np,K", SHAPES)
def test_tallk_product_and_bias_sums(dev, M, Np, K, transposed, gscale):
    _case(dev, M, Np, K, transposed, gscale, with_bias=transposed)


@pytest.mark.parametrize("max_splits", [1, 3])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("M,Np,K", SHAPES[2:])
def test_tallk_long_row_ranges(dev, M, Np, K, transposed, max_splits):
    """On a whole chip the split leaves these small shapes one or two 64-row blocks per workgroup; capped ("tallk_wgrad_max_splits"), a workgroup
    walks 13 or 38 blocks: the accumulation sign flips inside its range (every 4 blocks), the staging ring wraps, the range is odd or even."""
    from piano_a2s_amd import hip
    L = hip.lib()
    prev = L.a2s_debug_get(b"tallk_wgrad_max_splits")
    try:
        hip.check(L.a2s_debug_set(b"tallk_wgrad_max_splits", max_splits), "debug_set")
        _case(dev, M, Np, K, transposed, 1.0, with_bias=True)
    finally:
        hip.check(L.a2s_debug_set(b"tallk_wgrad_max_splits", prev), "debug_set")


@pytest.mark.parametrize("p_wide,a_wide,g_wide", [(True, False, False), (False, True, False), (False, False, True), (True, True, True)])
@pytest.mark.parametrize("transposed", [False, True])
def test_tallk_strided_operands_and_output(dev, transposed, p_wide, a_wide, g_wide):
    _case(dev, 327, 256, 256, transposed, 1.0, p_wide=p_wide, a_wide=a_wide, g_wide=g_wide, with_bias=True)


def test_switch_off_reports_ineligible(dev):
    from piano_a2s_amd import hip
    L = hip.lib()
    prev = L.a2s_debug_get(b"tallk_wgrad")
    try:
        hip.check(L.a2s_debug_set(b"tallk_wgrad", 0), "debug_set")
        assert L.a2s_tallk_wgrad_eligible(327, 256, 256, 256, 256, 256, 0) == 0
        x = torch.ones(327, 256, device=dev)
        G = torch.zeros(256, 256, device=dev)
        assert not hip.tallk_wgrad(x, 0, 256, x, 0, 256, G, 0, 256, 327, 256, 256, hip.one(dev), hip.one(dev))
        assert not bool(G.any())
    finally:
        hip.check(L.a2s_debug_set(b"tallk_wgrad", prev), "debug_set")
    assert L.a2s_tallk_wgrad_eligible(327, 256, 256, 256, 256, 256, 0) == 1
    assert L.a2s_tallk_wgrad_eligible(327, 128, 256, 128, 256, 256, 0) == 0          # the packed operand comes in blocks of 256 columns
    assert L.a2s_tallk_wgrad_eligible(327, 256, 192, 256, 192, 192, 0) == 0          # the staged one in tiles of 128
    assert L.a2s_tallk_wgrad_eligible(63, 256, 256, 256, 256, 256, 0) == 0


def test_linear_weight_gradient_bits_unchanged(dev):
    """The 19200 -> 256 Linear's own call, at the (64 * 37 + 5, 6, 64, 1.0) shape of test_linear_weight_gradient_kernel: G is bit-identical to the one
    recorded from the library before lin_wgrad_roles took the tall-K products as well."""
    import numpy as np
    from piano_a2s_amd import hip
    M, channels, period, gscale = 64 * 37 + 5, 6, 64, 1.0
    K, N = channels * period, 256
    g = torch.Generator().manual_seed(M + K)
    y = (torch.randn(M, K, generator=g) * 2.0).to(dev)
    dz = (torch.randn(M, N, generator=g) * gscale).to(dev)
    dz[M // 3] *= 2.0 ** -12
    scale = (torch.randn(channels, generator=g)).to(dev)
    shift = (torch.randn(channels, generator=g) * 0.3).to(dev)
    ymax = y.view(M, channels, period).abs().amax(dim=(0, 2)).contiguous()
    bound, dmax = hip.act_bound(scale, shift, ymax), hip.absmax(dz)
    G = (torch.randn(N, K, generator=g) * gscale).to(dev)
    assert hip.linear_wgrad(dz, y, (scale, shift, period), dmax, bound, G)
    torch.cuda.synchronize()
    want = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "lin_wgrad_parent_2373x384.npy")))
    assert torch.equal(G.cpu(), want)
