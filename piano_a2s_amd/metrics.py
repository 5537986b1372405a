"""Validation metrics of the recipe (reference pretrain.py:216-249): word error rate over ``" \\n = \\n "``-joined bars of
space-joined Kern symbols (the reference calls jiwer.wer -- third-party, absent here: restated as word-level Levenshtein distance
/ reference length, jiwer's definition), and macro-F1 of key / time-signature ids (sklearn.metrics.f1_score, as the reference).

The distances of corpus_wer come from the device (csrc/a2s_metrics.hip: one launch over all clips of the stage) once the process has the GPU
open, and from the host loop below otherwise; the floats are the same Python expressions either way.  macro-F1 stays on the host (sklearn per
clip, a few ms: its float parity with sklearn is not worth risking; a possible follow-up)."""
import os
import sys
import time

import numpy as np

from .spec import EOS

BAR_JOIN = " \n = \n "


def word_error_rate(reference, hypothesis):
    """(substitutions + deletions + insertions) / number of reference words, on whitespace-split words."""
    r, h = reference.split(), hypothesis.split()
    if not r:
        return float(len(h) > 0)
    prev = list(range(len(h) + 1))
    for i, rw in enumerate(r, 1):
        cur = [i] + [0] * len(h)
        for j, hw in enumerate(h, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (rw != hw))
        prev = cur
    return prev[-1] / len(r)


def unpad(ids):
    """Token row -> ids before the first <eos> (reference pretrain.py:245-249)."""
    ids = np.asarray(ids)
    hit = np.nonzero(ids == EOS)[0]
    return ids[: hit[0]] if len(hit) else ids


def ids_to_text(rows, inv_map):
    return BAR_JOIN.join(" ".join(inv_map[int(i)] for i in row) for row in rows)


# corpus_wer takes its distances from the device when this is true, the library is built and the process has initialised the GPU already
# (the model ran there): scoring never opens a GPU context by itself.  A2S_WER_DEVICE=0: always the host loop.
WER_DEVICE = os.environ.get("A2S_WER_DEVICE", "1") != "0"
# what the last corpus_wer call did: {"backend": "device" | "host", "pairs", "device_pairs", "host_pairs", "seconds"}; on the device path also
# "pack_seconds" (ids -> word codes on the host) and "device_seconds" (transfers + kernel)
last_wer_stats = {}


def _word_lookup(inv_map, table):
    """Per id the codes of inv_map[id].split() (zero, one or several words), as CSR arrays indexed by id; count -1: id not in inv_map."""
    n = max(inv_map, default=-1) + 1
    start, count, codes = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64), []
    for i, text in inv_map.items():
        words = text.split()
        start[i], count[i] = len(codes), len(words)
        codes.extend(table.setdefault(w, len(table)) for w in words)
    return start, count, np.asarray(codes, dtype=np.int32)


def pack_words(rows_per_clip, inv_map, table=None):
    """rows_per_clip: per clip its list of per-bar id rows.  Returns (words int32, offsets int64, table): clip c's slice
    words[offsets[c]:offsets[c + 1]] holds, as codes of `table` (word -> code, extended here; share it between the two sides of a
    comparison), exactly the words of ``ids_to_text(rows, inv_map).split()``: per id the words of its text, one "=" between consecutive bars."""
    if table is None:
        table = {}
    start, count, codes = _word_lookup(inv_map, table)
    eq = table.setdefault("=", len(table))
    n_clips = len(rows_per_clip)
    bars = [np.asarray(bar, dtype=np.int64).reshape(-1) for clip in rows_per_clip for bar in clip]
    clip_bars = np.fromiter((len(clip) for clip in rows_per_clip), dtype=np.int64, count=n_clips)
    bar_len = np.fromiter((b.size for b in bars), dtype=np.int64, count=len(bars))
    ids = np.concatenate(bars) if bars else np.zeros(0, dtype=np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= len(count) or (count[ids] < 0).any()):
        raise KeyError(f"pack_words: id without a symbol in inv_map among {np.unique(ids)[:8].tolist()}...")
    c = count[ids]                                                   # words per token
    if (c == 1).all():
        words = codes[start[ids]]
    else:                                                            # whitespace symbols (no word) or symbols of several words
        first = np.cumsum(c) - c
        words = codes[np.repeat(start[ids] - first, c) + np.arange(int(c.sum()))]
    csum = np.concatenate(([0], np.cumsum(c)))
    bar_end = np.cumsum(bar_len)
    bar_words = csum[bar_end] - csum[bar_end - bar_len]
    # a clip of nb bars has nb - 1 separators (also between empty bars); bar k of a clip lies behind k of them
    clip_seps = np.maximum(clip_bars - 1, 0)
    clip_first_bar = np.cumsum(clip_bars) - clip_bars
    bar_clip = np.repeat(np.arange(n_clips), clip_bars)
    sep_before = (np.cumsum(clip_seps) - clip_seps)[bar_clip] + np.arange(len(bars)) - clip_first_bar[bar_clip]
    out = np.full(len(words) + int(clip_seps.sum()), eq, dtype=np.int32)
    out[np.arange(len(words)) + np.repeat(sep_before, bar_words)] = words
    wsum = np.concatenate(([0], np.cumsum(bar_words)))
    clip_words = wsum[clip_first_bar + clip_bars] - wsum[clip_first_bar] + clip_seps
    return out, np.concatenate(([0], np.cumsum(clip_words))).astype(np.int64), table


def edit_distance_capacity():
    """Longest sequence (in words) the device kernel takes."""
    from . import hip
    return int(hip.lib().a2s_edit_distance_max_len())


def edit_distances(ref_words, ref_off, hyp_words, hyp_off, device=None):
    """Unit-cost Levenshtein distance of every pair (ref_words[ref_off[p]:ref_off[p + 1]], hyp_words[hyp_off[p]:hyp_off[p + 1]]) as a numpy
    int array: one host-to-device copy, one launch on the current stream of `device` (default: the current one), one copy back."""
    import torch
    from . import hip
    L = hip.lib()
    if not hasattr(L, "a2s_edit_distance"):
        raise hip.A2SError(f"{hip.LIB} has no a2s_edit_distance (a build from before the device-side scoring)")
    ref_off, hyp_off = np.asarray(ref_off, dtype=np.int64), np.asarray(hyp_off, dtype=np.int64)
    n = len(ref_off) - 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    rl, hl = np.diff(ref_off), np.diff(hyp_off)
    # longest first: a pair costs (rows = the shorter side) x (registers per lane = the longer side's bucket)
    epl = 4 << np.searchsorted(np.array([256, 512, 1024]), np.maximum(rl, hl), side="left")
    order = np.argsort(-(np.minimum(rl, hl) * (5 * epl + 12)), kind="stable")
    nr, nh = int(ref_off[-1]), int(hyp_off[-1])
    buf = np.empty(4 * (n + 1) + n + nr + nh, dtype=np.int32)        # [ref_off | hyp_off] as int64, then order, ref words, hyp words
    off64 = buf[:4 * (n + 1)].view(np.int64)
    off64[:n + 1], off64[n + 1:] = ref_off, hyp_off
    w = 4 * (n + 1)
    buf[w:w + n] = order
    buf[w + n:w + n + nr] = ref_words[:nr]
    buf[w + n + nr:] = hyp_words[:nh]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        d_in = torch.from_numpy(buf).to(dev)
        dist = torch.empty(n, dtype=torch.int32, device=dev)
        base = d_in.data_ptr()
        hip.check(L.a2s_edit_distance(hip.stream(), base + 16 * (n + 1) + 4 * n, base, base + 16 * (n + 1) + 4 * (n + nr), base + 8 * (n + 1),
                                      base + 16 * (n + 1), n, int(rl.max()), int(hl.max()), dist.data_ptr()), "a2s_edit_distance")
        out = dist.cpu().numpy().astype(np.int64)                    # (the copy waits for the launch: d_in stays referenced until here)
    if (out < 0).any():
        raise hip.A2SError("a2s_edit_distance: the offsets describe a pair beyond the kernel's capacity")
    return out


def _device_ready():
    torch = sys.modules.get("torch")                                 # not imported -> the GPU cannot have been opened
    if not WER_DEVICE or torch is None or not torch.cuda.is_initialized():
        return False
    from .build import LIB
    return os.path.exists(os.environ.get("A2S_LIB", LIB))


def _host_wer(k, pred, target, inv_map):
    return word_error_rate(ids_to_text(target[k], inv_map), ids_to_text(pred[k], inv_map))


def _csr_take(words, off, idx):
    lens = (off[1:] - off[:-1])[idx]
    return (np.concatenate([words[off[i]:off[i + 1]] for i in idx] + [np.zeros(0, dtype=np.int32)]),
            np.concatenate(([0], np.cumsum(lens))).astype(np.int64))


def corpus_wer(pred, target, inv_map):
    """pred/target: dict id -> list of per-bar id lists.  Returns (mean WER over clips, per-clip dict)."""
    global last_wer_stats
    t0 = time.perf_counter()
    keys = list(pred)
    if not keys or not _device_ready():
        per = {k: _host_wer(k, pred, target, inv_map) for k in keys}
        last_wer_stats = {"backend": "host", "pairs": len(keys), "device_pairs": 0, "host_pairs": len(keys), "seconds": time.perf_counter() - t0}
        return (sum(per.values()) / max(len(per), 1)), per
    ref_w, ref_o, table = pack_words([target[k] for k in keys], inv_map)
    hyp_w, hyp_o, table = pack_words([pred[k] for k in keys], inv_map, table)
    t1 = time.perf_counter()
    rl, hl = np.diff(ref_o), np.diff(hyp_o)
    cap = edit_distance_capacity()
    on_dev = np.nonzero((rl <= cap) & (hl <= cap))[0]
    dist = np.full(len(keys), -1, dtype=np.int64)
    if len(on_dev) == len(keys):
        dist[:] = edit_distances(ref_w, ref_o, hyp_w, hyp_o)
    elif len(on_dev):                                                # (a max_length beyond the shipped hparams: the long pairs stay on the host)
        dist[on_dev] = edit_distances(*_csr_take(ref_w, ref_o, on_dev), *_csr_take(hyp_w, hyp_o, on_dev))
    t2 = time.perf_counter()
    per = {}
    for k, d, nr, nh in zip(keys, dist.tolist(), rl.tolist(), hl.tolist()):
        if d < 0:
            per[k] = _host_wer(k, pred, target, inv_map)
        else:
            per[k] = d / nr if nr else float(nh > 0)
    last_wer_stats = {"backend": "device", "pairs": len(keys), "device_pairs": len(on_dev), "host_pairs": len(keys) - len(on_dev),
                      "seconds": time.perf_counter() - t0, "pack_seconds": t1 - t0, "device_seconds": t2 - t1}
    return (sum(per.values()) / max(len(per), 1)), per


def corpus_f1(pred, target):
    from sklearn.metrics import f1_score
    per = {k: float(f1_score(target[k], pred[k], average="macro")) for k in pred}
    return (sum(per.values()) / max(len(per), 1)), per
