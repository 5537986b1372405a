"""Validation metrics of the recipe (reference pretrain.py:216-249): word error rate over ``" \\n = \\n "``-joined bars of
space-joined Kern symbols (the reference calls jiwer.wer -- third-party, absent here: restated as word-level Levenshtein distance
/ reference length, jiwer's definition), and macro-F1 of key / time-signature ids (sklearn.metrics.f1_score, as the reference).

The distances of corpus_wer come from the device (csrc/a2s_metrics.hip: one launch over all clips of the stage) once the process has the GPU
open, and from the host loop below otherwise; the floats are the same Python expressions either way.  macro-F1 stays on the host (sklearn per
clip, a few ms: its float parity with sklearn is not worth risking; a possible follow-up).

Not in the reference: the note-level precision / recall / F1 of the decoded bars (note_events .. corpus_note_f1 below), whose
counts come from csrc/a2s_notes.hip under the same rule and from the host definition otherwise."""
import os
import sys
import time
from itertools import chain

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


# ---------------------------------------------------------------------------------------------------------------- note-level F1
# Prediction and target are aligned bar by bar already (one decoder row per bar and staff): each row is parsed into notes (onset tick, MIDI number,
# duration ticks, pitch token) and the two multisets of a bar are intersected at four levels.  `note_events` below IS the definition; the device
# (csrc/a2s_notes.hip) restates it.  Everything up to the final divisions is integer arithmetic, so the two agree exactly.
NOTE_W = 147840                       # ticks of a whole note = 128 * 3 * 5 * 7 * 11: every duration symbol of the vocabulary is a whole number of ticks
NOTE_FIELDS = 8                       # spines of a bar row that are timed; events in later ones are dropped and flag the row
NOTE_REST = -2                        # midi table: the rest (-1: no pitch symbol)
NOTE_CLS = {"TAB": 1, "NL": 2, "FERM": 3, "CLOSE": 4, "EOS": 5, "PAD": 6, "SOS": 6}          # cls table (A2S_NOTE_CLS_* of include/a2s.h); every other class: 0
NOTE_COLUMNS = ("n_ref", "n_hyp", "tp_pitch", "tp_onset", "tp_value", "tp_spelled", "flags")
# corpus_note_f1 takes its counts from the device when this is true AND the rule of the WER holds (_device_ready: the process has the GPU open, the library
# is built, WER_DEVICE is on).  So A2S_WER_DEVICE=0 sends both metrics to the host: one switch for "scoring on the device", no second variable.
NOTE_DEVICE = True
# what the last corpus_note_f1 / note_match call did: {"backend": "device" | "host", "rows" (bar pairs), "device_rows", "host_rows", "seconds"}; on the
# device path also "pack_seconds" and "device_seconds" (transfers + kernel)
last_note_stats = {}
_note_tables = None
_note_device_tables = {}


def note_tables():
    """{"W", "dur_ticks", "midi", "cls"}: per id of LabelsMultiple(extended=True) the ticks of a duration symbol (0: not one), the MIDI number of a
    pitch symbol (NOTE_REST for `r`, -1: not one) and the class code of NOTE_CLS, as read-only int32 arrays.  Derived from the symbols by pattern
    (kern_grammar.token_class, kern_transpose.parse_pitch), never from literal ids."""
    global _note_tables
    if _note_tables is None:
        from data_processing.humdrum import LabelsMultiple
        from .kern_grammar import token_class
        from .kern_transpose import parse_pitch
        labels = LabelsMultiple(extended=True).labels
        dur, midi, cls = np.zeros(len(labels), dtype=np.int32), np.full(len(labels), -1, dtype=np.int32), np.zeros(len(labels), dtype=np.int32)
        for i, sym in enumerate(labels):
            c = token_class(sym)
            if c == "DUR":                                       # reciprocal r: W / r ticks; dotted: 3 W / (2 r)
                dotted = sym.endswith(".")
                num, den = NOTE_W * (3 if dotted else 1), int(sym.rstrip(".")) * (2 if dotted else 1)
                assert den > 0 and num % den == 0, f"duration symbol {sym!r} is not a whole number of ticks"
                dur[i] = num // den
            elif c == "PITCH":
                midi[i] = NOTE_REST if sym == "r" else parse_pitch(sym)[1]
            else:
                cls[i] = NOTE_CLS.get(c, 0)
        assert dur.max() < 1 << 18 and midi.max() < 1 << 7          # the device packs a note as onset << 25 | midi << 18 | ticks
        for t in (dur, midi, cls):
            t.setflags(write=False)
        _note_tables = {"W": NOTE_W, "dur_ticks": dur, "midi": midi, "cls": cls}
    return _note_tables


note_tables()                         # (the assertions hold at import)


def _note_parse(ids_row):
    """-> (events [(line, field, ticks, midi, token id, continuation)] in row order, line times {line: onset}, overflow)."""
    tb = note_tables()
    dur, midi, cls = tb["dur_ticks"], tb["midi"], tb["cls"]
    V, ign, eos = len(dur), NOTE_CLS["PAD"], NOTE_CLS["EOS"]
    row = []
    for t in np.asarray(ids_row, dtype=np.int64).reshape(-1).tolist():
        if 0 <= t < V:
            if cls[t] == eos:
                break
            if cls[t] != ign:
                row.append(t)
    events, line, field = [], 0, 0
    for i, t in enumerate(row):
        c = cls[t]
        if c == NOTE_CLS["NL"]:
            line, field = line + 1, 0
        elif c == NOTE_CLS["TAB"]:
            field += 1
        elif midi[t] != -1 and i > 0 and dur[row[i - 1]] > 0:
            nxt = row[i + 1:i + 3]
            if nxt and cls[nxt[0]] == NOTE_CLS["FERM"]:
                nxt = nxt[1:]
            events.append((line, field, int(dur[row[i - 1]]), int(midi[t]), t, bool(nxt) and cls[nxt[0]] == NOTE_CLS["CLOSE"]))
    overflow = any(e[1] >= NOTE_FIELDS for e in events)
    end, t, times, i = [0] * NOTE_FIELDS, 0, {}, 0
    while i < len(events):
        j, first = i, {}
        while j < len(events) and events[j][0] == events[i][0]:
            if events[j][1] < NOTE_FIELDS:
                first.setdefault(events[j][1], events[j][2])     # per field of this line the ticks of its first event
            j += 1
        if first:
            t = max(t, min(end[f] for f in first))
            for f, ticks in first.items():
                end[f] = t + ticks
        times[events[i][0]] = t
        i = j
    return events, times, overflow


def note_events(ids_row):
    """THE DEFINITION.  One bar row of token ids -> (notes [(onset tick, MIDI number, duration ticks, pitch token id)] in row order, overflow).
    The row ends before its first <eos>; <pad>, <sos> and ids outside the vocabulary are taken out.  An event is a PITCH-class token (the rest
    included) that directly follows a DUR token; its line is the number of NL tokens before it, its field the number of TAB tokens since the last NL.
    It is a continuation if the token behind it -- behind one optional fermata -- is `_` or `]`.  A note is an event that is neither a rest nor a
    continuation.  Time: end[j] = 0 for the fields j < 8; line by line, t = max(t_prev, min of end[j] over the fields of the line that hold an
    event), then end[j] = t + the ticks of the field's first event; every note of the line starts at t with its own duration.  A line without
    events changes nothing.  Events in fields >= 8 are dropped and set `overflow`.  Tied chains are not merged: `[4c` then `4c]` is one quarter."""
    events, times, overflow = _note_parse(ids_row)
    return [(times[l], m, ticks, tok) for l, f, ticks, m, tok, cont in events if m != NOTE_REST and not cont and f < NOTE_FIELDS], overflow


def _multiset_overlap(a, b):
    from collections import Counter
    ca, cb = Counter(a), Counter(b)
    return sum(min(n, cb[k]) for k, n in ca.items())


def note_counts(ref_row, hyp_row):
    """The host counts of one pair of bar rows (target, prediction), as NOTE_COLUMNS: note counts of the two sides, the sizes of the multiset
    intersections keyed by MIDI number / (onset, MIDI) / (onset, MIDI, ticks) / (onset, pitch token), flags (bit 0: the target row overflowed the
    eight spines, bit 1: the prediction row)."""
    r, ro = note_events(ref_row)
    h, ho = note_events(hyp_row)
    return (len(r), len(h), _multiset_overlap([n[1] for n in r], [n[1] for n in h]), _multiset_overlap([n[:2] for n in r], [n[:2] for n in h]),
            _multiset_overlap([n[:3] for n in r], [n[:3] for n in h]), _multiset_overlap([(n[0], n[3]) for n in r], [(n[0], n[3]) for n in h]),
            int(ro) | int(ho) << 1)


def note_match_capacity():
    """Longest bar row (in ids) the device kernel takes."""
    from . import hip
    return int(hip.lib().a2s_note_match_max_len())


def _pair_rows(ref_rows_per_clip, hyp_rows_per_clip):
    """Bars are paired by index; a bar that one side lacks is paired with an empty row.  -> (ref rows, hyp rows, pairs per clip)."""
    ref, hyp, per_clip = [], [], []
    for r, h in zip(ref_rows_per_clip, hyp_rows_per_clip):
        n = max(len(r), len(h))
        ref += list(r) + [()] * (n - len(r))
        hyp += list(h) + [()] * (n - len(h))
        per_clip.append(n)
    return ref, hyp, np.asarray(per_clip, dtype=np.int64)


def _sum_clips(pair_counts, per_clip):
    """(pairs, 7) counts -> (clips, 7): the six counts summed over a clip's bars, the last column its number of overflowed rows."""
    c = np.asarray(pair_counts, dtype=np.int64).reshape(-1, len(NOTE_COLUMNS)).copy()
    c[:, 6] = (c[:, 6] & 1) + (c[:, 6] >> 1 & 1)
    out = np.zeros((len(per_clip), len(NOTE_COLUMNS)), dtype=np.int64)
    has = per_clip > 0
    if has.any():
        out[has] = np.add.reduceat(c, (np.cumsum(per_clip) - per_clip)[has], axis=0)
    return out


def _csr_rows(rows):
    """Rows (sequences of ids) -> (ids int32, offsets int64), in one pass over the tokens: an array per row costs four times as much."""
    lens = np.fromiter(map(len, rows), dtype=np.int64, count=len(rows))
    ids = np.fromiter(chain.from_iterable(rows), dtype=np.int32, count=int(lens.sum()))
    return ids, np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def device_note_counts(ref_ids, ref_off, hyp_ids, hyp_off, device=None):
    """Device counts of every pair (ref_ids[ref_off[p]:ref_off[p + 1]], hyp_ids[hyp_off[p]:hyp_off[p + 1]]) as an (n, 8) numpy int32 array (the
    kernel's rows: NOTE_COLUMNS and a spare; -1 in the six counts of a pair beyond the capacity): one host-to-device copy, one launch on the current
    stream of `device` (default: the current one), one copy back."""
    import torch
    from . import hip
    L = hip.lib()
    if not hasattr(L, "a2s_note_match"):
        raise hip.A2SError(f"{hip.LIB} has no a2s_note_match (a build from before the note-level scoring)")
    ref_off, hyp_off = np.asarray(ref_off, dtype=np.int64), np.asarray(hyp_off, dtype=np.int64)
    n = len(ref_off) - 1
    if n <= 0:
        return np.zeros((0, 8), dtype=np.int32)
    nr, nh = int(ref_off[-1]), int(hyp_off[-1])
    buf = np.empty(4 * (n + 1) + nr + nh, dtype=np.int32)           # [ref_off | hyp_off] as int64, then the ref ids, the hyp ids
    off64 = buf[:4 * (n + 1)].view(np.int64)
    off64[:n + 1], off64[n + 1:] = ref_off, hyp_off
    w = 4 * (n + 1)
    buf[w:w + nr] = ref_ids[:nr]
    buf[w + nr:] = hyp_ids[:nh]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        tabs = _note_device_tables.get(str(dev))
        if tabs is None:                                             # the three vocabulary tables: uploaded once per device
            tb = note_tables()
            tabs = _note_device_tables[str(dev)] = tuple(torch.from_numpy(tb[k].copy()).to(dev) for k in ("dur_ticks", "midi", "cls"))
        d_in = torch.from_numpy(buf).to(dev)
        out = torch.empty((n, 8), dtype=torch.int32, device=dev)
        base = d_in.data_ptr()
        hip.note_match(base + 4 * w, base, base + 4 * (w + nr), base + 8 * (n + 1), n, *tabs, out)
        return out.cpu().numpy()                                     # (the copy waits for the launch: d_in stays referenced until here)


def note_match(ref_rows_per_clip, hyp_rows_per_clip, device=None):
    """Per clip the counts of NOTE_COLUMNS (an (n_clips, 7) int64 array; the last column: overflowed rows), summed over its bar pairs on the host
    -- no atomics, the sums are reproducible.  The pairs go to the device in one call (device_note_counts); a pair the kernel refuses (a row beyond
    its capacity) is scored by note_counts.  Fills last_note_stats."""
    global last_note_stats
    t0 = time.perf_counter()
    ref, hyp, per_clip = _pair_rows(ref_rows_per_clip, hyp_rows_per_clip)
    ref_ids, ref_off = _csr_rows(ref)
    hyp_ids, hyp_off = _csr_rows(hyp)
    t1 = time.perf_counter()
    raw = device_note_counts(ref_ids, ref_off, hyp_ids, hyp_off, device)
    t2 = time.perf_counter()
    counts = raw[:, :len(NOTE_COLUMNS)].astype(np.int64)
    host = np.nonzero(raw[:, 0] < 0)[0]
    for p in host.tolist():
        counts[p] = note_counts(ref[p], hyp[p])
    last_note_stats = {"backend": "device", "rows": len(ref), "device_rows": len(ref) - len(host), "host_rows": len(host),
                       "seconds": time.perf_counter() - t0, "pack_seconds": t1 - t0, "device_seconds": t2 - t1}
    return _sum_clips(counts, per_clip)


def _ratio(num, den):
    return num / den if den else 1.0


def note_scores(c):
    """One row of NOTE_COLUMNS sums -> the floats of a clip: F1 = 2 tp / (n_ref + n_hyp), precision tp / n_hyp, recall tp / n_ref at the three
    levels (1.0 where the denominator is 0), spelled_share = tp_spelled / tp_onset, and the integers they come from."""
    n_ref, n_hyp, tp_pitch, tp_onset, tp_value, tp_spelled, over = (int(v) for v in c)
    out = {}
    for level, tp in (("pitch", tp_pitch), ("onset", tp_onset), ("value", tp_value)):
        out["f1_" + level] = _ratio(2 * tp, n_ref + n_hyp)
        out["precision_" + level] = _ratio(tp, n_hyp)
        out["recall_" + level] = _ratio(tp, n_ref)
    out["spelled_share"] = _ratio(tp_spelled, tp_onset)
    out.update(n_ref=n_ref, n_hyp=n_hyp, tp_pitch=tp_pitch, tp_onset=tp_onset, tp_value=tp_value, tp_spelled=tp_spelled, overflow_rows=over)
    return out


NOTE_MEAN_KEYS = ("f1_pitch", "f1_onset", "f1_value", "spelled_share", "precision_pitch", "precision_onset", "precision_value", "recall_pitch",
                  "recall_onset", "recall_value")


def corpus_note_f1(pred, target):
    """pred/target: dict id -> list of per-bar id rows (one staff), as corpus_wer takes them.  Returns (means, per_clip): per clip the dict of
    note_scores, `means` the means over the clips of its floats and the total of overflow_rows."""
    global last_note_stats
    t0 = time.perf_counter()
    keys = list(pred)
    if keys and NOTE_DEVICE and _device_ready():
        sums = note_match([target[k] for k in keys], [pred[k] for k in keys])
        last_note_stats["seconds"] = time.perf_counter() - t0
    else:
        ref, hyp, per_clip = _pair_rows([target[k] for k in keys], [pred[k] for k in keys])
        sums = _sum_clips([note_counts(r, h) for r, h in zip(ref, hyp)], per_clip)
        last_note_stats = {"backend": "host", "rows": len(ref), "device_rows": 0, "host_rows": len(ref), "seconds": time.perf_counter() - t0}
    per = {k: note_scores(row) for k, row in zip(keys, sums)}
    means = {m: (sum(v[m] for v in per.values()) / len(per) if per else 1.0) for m in NOTE_MEAN_KEYS}
    means["overflow_rows"] = sum(v["overflow_rows"] for v in per.values())
    return means, per
