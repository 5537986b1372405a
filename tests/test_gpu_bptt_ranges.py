"""The operand ranges the persistent BPTT launch hands out (csrc/a2s_persist.hip, gru_seq_bwd_persist: wave 0 keeps max |.| of what it writes to
dgi_all and dgh_shift; a2s_gru_seq_bwd_ranged copies the two words out of the launch's workspace header): bit-equal to a2s_absmax of the two tensors,
in both directions, at the smallest shapes tests/test_gpu_persist.py runs the kernel at and at batch sizes that are no multiple of the 16-row tile;
the gradients themselves are the bits a2s_gru_seq_bwd writes, with the "tallk_wgrad" switch off and on; the launch-per-step kernels report no ranges."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _forward(L, hip, dev, gi, w_hh, b_hh, B, T, H, d):
    ws = hip.gru_workspace(B, H, dev)      # W_hh^T + the persistent launches' granule buffers
    out = torch.zeros(B, T, 2 * H, device=dev)
    hbuf, gh, hn = torch.empty(2, B, H, device=dev), torch.empty(B, 3 * H, device=dev), torch.empty(B, H, device=dev)
    gates = torch.empty(T, B, 4 * H, device=dev)
    hip.check(L.a2s_gru_seq_fwd(hip.stream(), hip._p(gi), C.c_long(T * 3 * H), C.c_long(3 * H), hip._p(w_hh), hip._p(b_hh),
                                C.c_void_p(out.data_ptr() + 4 * d * H), C.c_long(T * 2 * H), C.c_long(2 * H), hip._p(hbuf), hip._p(gh), hip._p(gates),
                                hip._p(hn), B, T, H, d, hip._p(ws), C.c_size_t(ws.numel() * 4)), "fwd")
    return out, gates, ws


def _backward(L, hip, dev, out, gates, ws, w_hh, dout, dhn, B, T, H, d, ranged):
    dgi, dghs = torch.full((B, T, 3 * H), float("nan"), device=dev), torch.full((B, T, 3 * H), float("nan"), device=dev)
    dgh_first, dhbuf, dgh_tmp = torch.empty(B, 3 * H, device=dev), torch.empty(2, B, H, device=dev), torch.empty(B, 3 * H, device=dev)
    args = (hip.stream(), C.c_void_p(dout.data_ptr() + 4 * d * H), C.c_long(T * 2 * H), C.c_long(2 * H), C.c_void_p(out.data_ptr() + 4 * d * H),
            C.c_long(T * 2 * H), C.c_long(2 * H), hip._p(gates), hip._p(w_hh), hip._p(dhn), hip._p(dgi), hip._p(dghs), hip._p(dgh_first), hip._p(dhbuf),
            hip._p(dgh_tmp), B, T, H, d, hip._p(ws), C.c_size_t(ws.numel() * 4))
    ranges, valid = torch.full((2,), float("nan"), device=dev), C.c_int(-1)
    if ranged:
        hip.check(L.a2s_gru_seq_bwd_ranged(*args, hip._p(ranges), C.byref(valid)), "bwd ranged")
    else:
        hip.check(L.a2s_gru_seq_bwd(*args), "bwd")
    torch.cuda.synchronize()
    return dgi, dghs, dgh_first, ranges, valid.value


@pytest.mark.parametrize("B,T", [(3, 2), (16, 5), (37, 29)])
def test_range_words_equal_absmax(dev, B, T):
    from piano_a2s_amd import hip
    L = hip.lib()
    H = 256
    g = torch.Generator().manual_seed(100 + B)
    prev_p, prev_t = L.a2s_debug_get(b"gru_persist"), L.a2s_debug_get(b"tallk_wgrad")
    try:
        for d in (0, 1):
            gi = (torch.randn(B, T, 3 * H, generator=g) * 0.8).to(dev)
            w_hh = (torch.randn(3 * H, H, generator=g) * 0.08).to(dev)
            b_hh = (torch.randn(3 * H, generator=g) * 0.1).to(dev)
            dout = (torch.randn(B, T, 2 * H, generator=g) * (1e-3 if d else 1.0)).to(dev)
            dhn = torch.randn(B, H, generator=g).to(dev)
            hip.check(L.a2s_debug_set(b"gru_persist", 1), "debug_set")
            out, gates, ws = _forward(L, hip, dev, gi, w_hh, b_hh, B, T, H, d)
            plain = _backward(L, hip, dev, out, gates, ws, w_hh, dout, dhn, B, T, H, d, ranged=False)
            for on in (0, 1):
                hip.check(L.a2s_debug_set(b"tallk_wgrad", on), "debug_set")
                dgi, dghs, dgh_first, ranges, valid = _backward(L, hip, dev, out, gates, ws, w_hh, dout, dhn, B, T, H, d, ranged=True)
                assert valid == 1, "the persistent launch reports its ranges"
                assert torch.isfinite(dgi).all() and torch.isfinite(dghs).all() and torch.isfinite(dgh_first).all()
                for name, a, b in (("dgi_all", dgi, plain[0]), ("dgh_shift", dghs, plain[1]), ("dgh_first", dgh_first, plain[2])):
                    assert torch.equal(a, b), f"direction {d} {name}: differs from a2s_gru_seq_bwd"
                want = torch.cat([hip.absmax(dgi), hip.absmax(dghs)])
                torch.cuda.synchronize()
                assert float(want[0]) > 0 and float(want[1]) > 0
                assert torch.equal(ranges.view(torch.int32), want.view(torch.int32)), f"direction {d}: range words {ranges.tolist()} against absmax {want.tolist()}"
            # the launch-per-step kernels: no range words, the same entry point
            hip.check(L.a2s_debug_set(b"gru_persist", 0), "debug_set")
            *_, ranges, valid = _backward(L, hip, dev, out, gates, ws, w_hh, dout, dhn, B, T, H, d, ranged=True)
            assert valid == 0 and bool(torch.isnan(ranges).all()), "no persistent launch: nothing reported, nothing written"
    finally:
        hip.check(L.a2s_debug_set(b"gru_persist", prev_p), "debug_set")
        hip.check(L.a2s_debug_set(b"tallk_wgrad", prev_t), "debug_set")
