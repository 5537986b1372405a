"""Scoring on the device (csrc/a2s_metrics.hip through metrics.edit_distances / metrics.corpus_wer): the distances are integers, so every
comparison here is equality -- against a plain Python table for the kernel, against the host loop for corpus_wer."""
import numpy as np
import pytest
import torch

from data_processing.humdrum import LabelsMultiple
from piano_a2s_amd import metrics, synthetic

pytestmark = pytest.mark.gpu

INV = LabelsMultiple(extended=True).labels_map_inv
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 513)        # lane and registers-per-lane boundaries


def _dp(r, h):
    prev = list(range(len(h) + 1))
    for i, rw in enumerate(r, 1):
        cur = [i] * (len(h) + 1)
        left = i
        for j, hw in enumerate(h, 1):
            left = cur[j] = min(prev[j] + 1, left + 1, prev[j - 1] + (rw != hw))
        prev = cur
    return prev[-1]


def _csr(seqs):
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
    words = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs] + [np.zeros(0, dtype=np.int32)])
    return words, off


def _lib():
    from piano_a2s_amd import hip
    return hip.lib()


@pytest.fixture(autouse=True)
def gpu_open():
    torch.zeros(1, device="cuda")                                # the model has run on the GPU: the precondition of the device path
    assert torch.cuda.is_initialized()


def test_kernel_against_python_table():
    rng = np.random.default_rng(7)
    word = lambda n, k=40: rng.integers(0, k, size=n).tolist()
    pairs = [(word(a), word(b)) for a in LENGTHS for b in LENGTHS]                        # 121 pairs, every bucket and both orientations
    for n in (1, 64, 200, 513):
        s = word(n)
        pairs.append((s, list(s)))                                                         # identical
        pairs.append((s, [w + 1000 for w in word(n + 3)]))                                 # no common word
    base = word(300, 12)
    for k in (1, 64, 65):                                                                  # the chain cur[j-1] + 1 across lanes and whole lanes
        ins = [w + 500 for w in word(k)]
        for at in (0, 150, 300):
            longer = base[:at] + ins + base[at:]
            pairs.append((base, longer))
            pairs.append((longer, base))
    for a, b in ((200, 200), (513, 400), (64, 65), (1000, 129)):                            # two words only: ties everywhere
        pairs.append((word(a, 2), word(b, 2)))
    big = [(2047, 2047), (2047, 1), (1, 2047), (1994, 354), (354, 1994), (2047, 0)]
    pairs += [(word(a, 150), word(b, 150)) for a, b in big]
    near = word(2047, 150)                                                                 # a long near-copy: small distance, long diagonal
    pairs.append((near, [w for i, w in enumerate(near) if i % 37]))
    L = _lib()
    before, counted = L.a2s_debug_get(b"edit_distance_launches"), L.a2s_launch_count()
    refs, hyps = _csr([p[0] for p in pairs]), _csr([p[1] for p in pairs])
    got = metrics.edit_distances(*refs, *hyps)
    assert L.a2s_debug_get(b"edit_distance_launches") == before + 1 and L.a2s_launch_count() == counted + 1     # one launch of mixed lengths
    expect = [_dp(r, h) for r, h in pairs]
    wrong = [(i, len(pairs[i][0]), len(pairs[i][1]), int(got[i]), expect[i]) for i in range(len(pairs)) if int(got[i]) != expect[i]]
    assert not wrong, f"{len(wrong)} of {len(pairs)} pairs (index, ref words, hyp words, device, table): {wrong[:10]}"
    assert got.tolist()[121] == 0 and got.tolist()[122] == 4


def test_full_capacity_and_refusal():
    from piano_a2s_amd import hip
    cap = metrics.edit_distance_capacity()
    assert cap >= 2047
    a, b = np.arange(cap, dtype=np.int32), np.arange(cap, dtype=np.int32) + 1              # shifted by one word: one deletion + one insertion
    got = metrics.edit_distances(*_csr([a, a, []]), *_csr([b, [], a]))
    assert got.tolist() == [2, cap, cap]
    with pytest.raises(hip.A2SError):
        metrics.edit_distances(*_csr([np.arange(cap + 1)]), *_csr([[1]]))
    torch.cuda.synchronize()


@pytest.mark.parametrize("hyp_set", ["near_copies", "no_eos"])
def test_corpus_wer_device_is_the_host_result(monkeypatch, hyp_set):
    corpus = synthetic.make_wer_corpus(64, 3)
    L = _lib()
    for staff in ("upper", "lower"):
        target, near, no_eos = corpus[staff]
        pred = near if hyp_set == "near_copies" else {k: [metrics.unpad(r).tolist() for r in rows] for k, rows in no_eos.items()}
        before = L.a2s_debug_get(b"edit_distance_launches")
        monkeypatch.setattr(metrics, "WER_DEVICE", True)
        dev = metrics.corpus_wer(pred, target, INV)
        stats = dict(metrics.last_wer_stats)
        assert stats["backend"] == "device" and stats["pairs"] == stats["device_pairs"] == 64 and stats["host_pairs"] == 0
        assert L.a2s_debug_get(b"edit_distance_launches") == before + 1
        monkeypatch.setattr(metrics, "WER_DEVICE", False)
        host = metrics.corpus_wer(pred, target, INV)
        assert metrics.last_wer_stats["backend"] == "host" and L.a2s_debug_get(b"edit_distance_launches") == before + 1
        assert dev == host and list(dev[1]) == list(host[1])                               # floats included, and the dict order
        assert all(type(v) is float for v in dev[1].values())
        if hyp_set == "no_eos":
            assert max(len(r) for rows in pred.values() for r in rows) == (398 if staff == "upper" else 189)
        print(f"{hyp_set} {staff}: device {stats['seconds'] * 1e3:.1f} ms (pack {stats['pack_seconds'] * 1e3:.1f}), host "
              f"{metrics.last_wer_stats['seconds'] * 1e3:.1f} ms, mean WER {dev[0]:.4f}")


def test_over_capacity_pair_goes_to_the_host_loop(monkeypatch):
    rng = np.random.default_rng(5)
    ids = np.array([i for i in range(140)])
    cap = metrics.edit_distance_capacity()
    target = {"a": [rng.choice(ids, 30).tolist() for _ in range(5)], "long": [rng.choice(ids, cap + 52).tolist()],
              "edge": [rng.choice(ids, cap).tolist()], "b": [[], rng.choice(ids, 7).tolist()], "none": []}
    pred = {"a": [r[:-2] for r in target["a"]], "long": [rng.choice(ids, 40).tolist()], "edge": [target["edge"][0][5:]],
            "b": [rng.choice(ids, 3).tolist(), []], "none": [[1]]}
    monkeypatch.setattr(metrics, "WER_DEVICE", True)
    dev = metrics.corpus_wer(pred, target, INV)
    stats = dict(metrics.last_wer_stats)
    assert stats["backend"] == "device" and stats["pairs"] == 5 and stats["host_pairs"] == 1 and stats["device_pairs"] == 4
    monkeypatch.setattr(metrics, "WER_DEVICE", False)
    host = metrics.corpus_wer(pred, target, INV)
    assert dev == host and list(dev[1]) == list(host[1])
    assert dev[1]["edge"] == 5 / cap and dev[1]["none"] == 1.0
    # ... and the other way round: the long side is the hypothesis
    monkeypatch.setattr(metrics, "WER_DEVICE", True)
    dev = metrics.corpus_wer(target, pred, INV)
    assert metrics.last_wer_stats["host_pairs"] == 1
    monkeypatch.setattr(metrics, "WER_DEVICE", False)
    assert dev == metrics.corpus_wer(target, pred, INV)


def test_call_leaves_nothing_behind(monkeypatch):
    monkeypatch.setattr(metrics, "WER_DEVICE", True)
    target, near, _ = synthetic.make_wer_corpus(16, 9)["lower"]
    first = metrics.corpus_wer(near, target, INV)
    torch.cuda.synchronize()
    assert metrics.last_wer_stats["backend"] == "device"
    second = metrics.corpus_wer(near, target, INV)
    assert first == second
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                                          # the caller's current stream, whichever it is
        third = metrics.corpus_wer(near, target, INV)
    torch.cuda.synchronize()
    assert third == first and metrics.last_wer_stats["host_pairs"] == 0
    assert metrics.corpus_wer({}, {}, INV) == (0.0, {})
