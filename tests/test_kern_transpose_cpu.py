"""The score side of the transposition augmentation on the host (piano_a2s_amd/kern_transpose.py, augment.TransposeAugment.draw):

1. the token map against the independent string-level transposer (tests/transpose_oracle.py), for all 25 (s, f) pairs x 173 tokens;
2. the key rule;
3. against the score generator: 60 clips x 13 shifts;
4. a hand-written chromatic bar;
5. the draws: range, reproducibility, no foreign random state advances."""
import random

import numpy as np
import pytest
import torch

from data_processing.humdrum import LabelsMultiple
from piano_a2s_amd import kern_transpose as kt
from piano_a2s_amd import scoregen, spec
from piano_a2s_amd.augment import TransposeAugment
from tests import transpose_oracle as oracle

LABELS = LabelsMultiple(extended=True)
SYMS = LABELS.labels
IDS = LABELS.labels_map
SHIFTS = range(-6, 7)


def test_vocabulary_has_136_pitch_tokens_and_25_intervals():
    assert len(SYMS) == 173 and kt.V == 173
    assert sum(oracle.parse(s) is not None for s in SYMS) == 136 and len(kt.PITCH_IDS) == 136
    assert {i for i, s in enumerate(SYMS) if oracle.parse(s) is not None} == set(kt.PITCH_IDS)
    assert len(kt.PAIRS) == 25 and kt.TOKEN_MAP.shape == (25, 173) and kt.TOKEN_MAP.dtype == np.int32
    assert all(-11 <= f <= 11 for _, f in kt.PAIRS)
    assert set(kt.PAIRS) == {(s, oracle.move_key(k, s) - k) for s in SHIFTS for k in range(-6, 8)}


# ------------------------------------------------------------------------------------------- 1. the token map
def test_token_map_equals_the_oracle_for_every_pair_and_token():
    undefined = 0
    for row, (s, f) in enumerate(kt.PAIRS):
        back = kt.PAIRS.index((-s, -f)) if (-s, -f) in kt.PAIRS else None
        for i, sym in enumerate(SYMS):
            got = int(kt.TOKEN_MAP[row, i])
            if oracle.parse(sym) is None:
                assert got == i, f"{sym!r} is no pitch: a fixed point of ({s}, {f})"
                continue
            want = oracle.move(sym, s, f)
            want_id = IDS.get(want, -1) if want is not None else -1
            assert got == want_id, f"{sym} by ({s}, {f}): {SYMS[got] if got >= 0 else None} != {want}"
            if got < 0:
                undefined += 1
                continue
            l0, a0, o0 = oracle.parse(sym)
            l1, a1, o1 = oracle.parse(SYMS[got])
            assert oracle.midi(l1, a1, o1) == oracle.midi(l0, a0, o0) + s
            assert oracle.position(l1, a1) == oracle.position(l0, a0) + f
            if back is not None:
                assert int(kt.TOKEN_MAP[back, got]) == i, f"{sym} by ({s}, {f}) and back"
    assert undefined > 0 and not (kt.TOKEN_MAP[kt.PAIRS.index((0, 0))] != np.arange(173)).any()


# ------------------------------------------------------------------------------------------- 2. the key rule
def test_key_rule():
    assert kt.NEW_KEY.shape == (13, 14) and kt.INTERVAL.shape == (13, 14)
    for s in SHIFTS:
        for k in range(-6, 8):
            k2 = int(kt.NEW_KEY[s + 6, k + 6]) - 6
            assert -6 <= k2 <= 7 and (k2 - k - 7 * s) % 12 == 0
            assert k2 == oracle.move_key(k, s)
            assert kt.PAIRS[int(kt.INTERVAL[s + 6, k + 6])] == (s, k2 - k)
            if s == 0:
                assert k2 == k
    quoted = {0: "6 1 -4 3 -2 5 0 -5 2 -3 4 -1 6", 7: "1 -4 3 -2 5 0 7 2 -3 4 -1 6 1", -6: "0 -5 2 -3 4 -1 -6 1 -4 3 -2 5 0"}
    for k, row in quoted.items():
        assert [int(kt.NEW_KEY[s + 6, k + 6]) - 6 for s in SHIFTS] == [int(v) for v in row.split()], k
    assert int(kt.NEW_KEY[1 + 6, 0 + 6]) - 6 == -5, "C major + 1 semitone is D flat major"
    assert int(kt.NEW_KEY[5 + 6, -6 + 6]) - 6 == 5, "G flat major + 5 semitones is B major"


# ------------------------------------------------------------------------------------------- 3. the score generator
# the two (seed, s) of 780 that the single-accidental alphabet cannot hold: both clips are in C sharp major, and bbb# + 6 semitones would be ffff#
UNREPRESENTABLE = {(4, 6), (41, 6)}


def test_generated_clips_stay_diatonic_and_text_and_ids_agree():
    cfg = spec.default_cfg()
    failed = set()
    for seed in range(60):
        clip = scoregen.make_clip(cfg, seed)
        key = clip["key"]
        for s in SHIFTS:
            scale = scoregen.key_scale(int(kt.NEW_KEY[s + 6, key]) - 6)
            for staff in ("upper", "lower"):
                for text, ids in zip(clip["text"][staff], clip["ids"][staff]):
                    by_ids, by_text = kt.transpose_ids(ids, key, s), kt.transpose_text(text, key, s)
                    assert (by_ids is None) == (by_text is None)
                    if by_ids is None:
                        failed.add((seed, s))
                        continue
                    assert by_ids[1] == by_text[1] == int(kt.NEW_KEY[s + 6, key])
                    assert LABELS.encode(by_text[0]) == by_ids[0]
                    assert len(by_ids[0]) == len(ids)
                    for old, new in zip(ids, by_ids[0]):
                        if old not in kt.PITCH_IDS:
                            assert new == old
                            continue
                        letter, alt, _ = oracle.parse(SYMS[new])
                        assert scale[letter.lower()] == alt, f"seed {seed}, s {s}: {SYMS[old]} -> {SYMS[new]} is not in the new key"
    assert failed == UNREPRESENTABLE, sorted(failed)
    for seed, s in UNREPRESENTABLE:
        clip = scoregen.make_clip(cfg, seed)
        assert clip["key"] - 6 == 7 and any(IDS["bbb#"] in ids for ids in clip["ids"]["upper"])


# ------------------------------------------------------------------------------------------- 4. a chromatic bar
def test_chromatic_bar_by_hand():
    c_major = 6
    text = "4e#\t[4c 4e\n8.r\t2GG_"
    ids = LABELS.encode(text)
    got, key = kt.transpose_ids(ids, c_major, 1)
    assert kt.PAIRS[int(kt.INTERVAL[1 + 6, c_major])] == (1, -5) and key == -5 + 6
    want_text = "4f#\t[4d- 4f\n8.r\t2AA-_"
    assert got == LABELS.encode(want_text)
    assert kt.transpose_text(text, c_major, 1) == (want_text, key)
    assert len(got) == len(ids) and all(a == b for a, b in zip(ids, got) if a not in kt.PITCH_IDS)
    sharp = text.replace("e#", "b#")
    assert kt.PAIRS[int(kt.INTERVAL[-1 + 6, c_major])] == (-1, 5)
    assert kt.transpose_ids(LABELS.encode(sharp), c_major, -1) is None and kt.transpose_text(sharp, c_major, -1) is None
    assert kt.transpose_ids(LABELS.encode(sharp), c_major, 1) is not None           # (b# by (1, -5) is c#)
    with pytest.raises(ValueError):
        kt.transpose_ids(ids, c_major, 7)
    with pytest.raises(ValueError):
        kt.transpose_ids(ids, 14, 1)


# ------------------------------------------------------------------------------------------- 5. the draws
def _states():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and torch.equal(a[2], b[2])


def test_draws_are_in_range_reproducible_and_private():
    before = _states()
    aug = TransposeAugment(spec.default_cfg(), 3, 1.5, seed=1234, device="cpu")
    aug.reseed(2, rank=0)
    s, d = aug.draw(4096)
    assert _same(before, _states()), "construction, reseed and draw leave Python's, numpy's and torch's generators alone"
    assert s.dtype == np.int32 and d.dtype == np.float32 and s.shape == d.shape == (4096,)
    assert set(s.tolist()) == set(range(-3, 4)) and -1.5 <= d.min() < -1.4 and 1.4 < d.max() <= 1.5
    again = TransposeAugment(spec.default_cfg(), 3, 1.5, seed=1234, device="cpu")
    again.draw(17)                                       # (what was drawn before the reseed does not matter)
    again.reseed(2, rank=0)
    s2, d2 = again.draw(4096)
    assert np.array_equal(s, s2) and np.array_equal(d, d2)
    for epoch, rank, seed in ((2, 1, 1234), (3, 0, 1234), (2, 0, 1235)):
        other = TransposeAugment(spec.default_cfg(), 3, 1.5, seed=seed, device="cpu")
        other.reseed(epoch, rank=rank)
        s3, d3 = other.draw(4096)
        assert not np.array_equal(s, s3) and not np.array_equal(d, d3), (epoch, rank, seed)
    only_s = TransposeAugment(spec.default_cfg(), 6, 0.0, seed=1, device="cpu").draw(64)
    assert (only_s[1] == 0).all() and set(only_s[0].tolist()) <= set(range(-6, 7))
    only_d = TransposeAugment(spec.default_cfg(), 0, 2.5, seed=1, device="cpu").draw(64)
    assert (only_d[0] == 0).all() and np.abs(only_d[1]).max() <= 2.5
    for K, D in ((7, 0), (-1, 0), (2.5, 0), (1, 2.6), (1, -0.1)):
        with pytest.raises(ValueError):
            TransposeAugment(spec.default_cfg(), K, D, seed=1, device="cpu")
    with pytest.raises(ValueError):
        TransposeAugment(spec.default_cfg(), 1, 0, seed=1, device="cpu", bins_per_octave=50)
