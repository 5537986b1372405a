"""From a recording to decoded bars (piano_a2s_amd/transcribe.py): what transcribe_waveform returns is what the model gives, run
by hand on VQT(cut_windows(Resampler(...))); the window plan, the n_bars trimming, the decoding options and the command line.  The model is the small
one of the other fixtures (seeded procedural weights: no trained checkpoint exists here) at the VQT's 480 bins."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(conv_feature_size=32, hidden_size=32, max_length=(12, 8))
HP = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
LENGTH = 192000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def state():
    from piano_a2s_amd import spec
    return spec.procedural_state(spec.default_cfg(**SMALL), 11, eos_bias=3.0, lively=True)


@pytest.fixture(scope="module")
def model(dev, state):
    import models
    m = models.ScoreTranscription(**SMALL)
    m.load_state_dict(state)
    return m.to(dev).eval()


@pytest.fixture()
def plain(model):
    """The module with its decoding options at their defaults, before and after."""
    def reset():
        model.constrained_decoding, model.beam_size, model.beam_length_penalty, model.alignment = False, 1, 0.0, False
    reset()
    yield model
    reset()


def _by_hand(model, windows):
    """(time signature ids, key ids, upper ids, lower ids) of the model on VQT(windows), as the recipe's evaluation reads them."""
    from piano_a2s_amd import transcribe
    feats = transcribe._vqt(windows.device, HP)(windows)
    with torch.no_grad():
        ts_o, key_o, up_o, lo_o = model(spectrogram=feats, inference=True, ground_truth=None, teacher_forcing_ratio=0., device=windows.device)
    if model.constrained_decoding or model.beam_size >= 2:
        up, lo = model.last_decoded["up"][0], model.last_decoded["lo"][0]
    else:
        up, lo = up_o.argmax(-1), lo_o.argmax(-1)
    return ts_o.argmax(-1).cpu().numpy(), key_o.argmax(-1).cpu().numpy(), up.cpu().numpy(), lo.cpu().numpy()


def _assert_windows(result, plan, hand):
    from piano_a2s_amd import metrics, transcribe
    inv, ts_list = transcribe.labels.labels_map_inv, transcribe.time_signatures()
    ts, key, up, lo = hand
    assert len(result["windows"]) == len(plan)
    for w, (win, (start, stop, n_bars)) in enumerate(zip(result["windows"], plan)):
        assert win["start_s"] == start / 16000 and win["stop_s"] == stop / 16000 and win["n_bars"] == n_bars
        assert len(win["bars"]) == n_bars == len(win["key"]) == len(win["time_signature"])
        assert win["key"] == [int(k) - 6 for k in key[w][:n_bars]] and win["time_signature"] == [ts_list[int(t)] for t in ts[w][:n_bars]]
        for i, bar in enumerate(win["bars"]):
            u, l = metrics.unpad(up[w][i]), metrics.unpad(lo[w][i])
            assert bar["upper_ids"] == u.tolist() and bar["lower_ids"] == l.tolist()
            assert bar["upper"] == metrics.ids_to_text([u], inv) and bar["lower"] == metrics.ids_to_text([l], inv)


@pytest.fixture(scope="module")
def rendered(dev):
    """12 s of a rendered clip (scoregen + render) at 16 kHz, scaled below full scale: (192000,) float32 on the host."""
    from piano_a2s_amd import scoregen, spec
    from piano_a2s_amd.render import render
    clip = scoregen.make_clip(spec.default_cfg(), 2024, frames=1201)
    w = render(torch.from_numpy(scoregen.pack_program(clip)[None]).to(dev))[0].cpu().numpy()
    assert w.shape == (LENGTH,) and np.abs(w).max() > 0
    return (w * (0.8 / np.abs(w).max())).astype(np.float32)


def _song(sr, seconds, channels, seed):
    """A few decaying partials every half second: (frames, channels) float32 in (-1, 1)."""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    x = np.zeros((n, channels))
    tt = np.arange(2 * sr) / float(sr)                                        # every note sounds for 2 s
    for onset in np.arange(0.25, seconds - 0.5, 0.5):
        f = 110.0 * 2.0 ** (rng.integers(0, 36) / 12.0)
        note = 0.12 * np.exp(-3.0 * tt) * np.hanning(2 * len(tt))[len(tt):] * (np.sin(2 * np.pi * f * tt) + 0.4 * np.sin(4 * np.pi * f * tt))
        i0 = int(round(onset * sr))
        i1 = min(n, i0 + len(tt))
        for c in range(channels):
            x[i0:i1, c] += (1.0 + 0.3 * c) * note[:i1 - i0]
    return np.clip(x, -0.99, 0.99).astype(np.float32)


# ------------------------------------------------------------------------------------------- one window at 16 kHz
def test_one_window_at_16k(tmp_path, dev, plain, rendered):
    from piano_a2s_amd import audio, transcribe
    path = tmp_path / "clip.wav"
    audio.write_wav(path, rendered, 16000, bits=16)
    x, sr = audio.read_wav(path)
    assert sr == 16000 and x.shape == (LENGTH, 1)
    assert np.array_equal(x[:, 0], (audio.quantise(rendered) / 32768.0).astype(np.float32))
    result = transcribe.transcribe_waveform(plain, x, sr, hparams=HP)
    assert result["sample_rate_in"] == 16000 and result["sample_rate"] == 16000 and result["frames_per_second"] == 100.0
    plan = [(0, LENGTH, 5)]
    w = audio.cut_windows(torch.from_numpy(x[:, 0]).to(dev), plan, LENGTH)
    hand = _by_hand(plain, w)
    _assert_windows(result, plan, hand)
    assert result["windows"][0]["flags"] == [] and "alignment" not in result["windows"][0]
    assert any(b["upper_ids"] for b in result["windows"][0]["bars"]), "the seeded model decodes something"


# ------------------------------------------------------------------------------------------- 48 kHz stereo with downbeats
def test_48k_stereo_with_downbeats(tmp_path, dev, plain):
    from piano_a2s_amd import audio, transcribe
    x = _song(48000, 30.0, 2, 1)
    path = tmp_path / "song.wav"
    audio.write_wav(path, x, 48000, bits=24)
    x, sr = audio.read_wav(path)
    assert sr == 48000 and x.shape == (1440000, 2)
    ann = tmp_path / "song_annotations.txt"
    times = [0.5 + 2.25 * i for i in range(13)]                               # 12 bars of 2.25 s: groups of 5, 5 and 2 bars
    lines = []
    for i, t in enumerate(times):
        lines.append(f"{t:.4f}\t{t:.4f}\tdb,4/4" if i == 0 else f"{t:.4f}\t{t:.4f}\tdb")
        lines.append(f"{t + 1.1:.4f}\t{t + 1.1:.4f}\tb")                      # a beat that is no downbeat: skipped
    ann.write_text("\n".join(lines) + "\n")
    downbeats = transcribe.read_downbeats(ann)
    assert downbeats == [float(f"{t:.4f}") for t in times]
    result = transcribe.transcribe_waveform(plain, x, sr, downbeats=downbeats, hparams=HP)
    wave, n_out = audio.Resampler(dev, 48000)(torch.from_numpy(x).to(dev)[None])
    assert n_out.tolist() == [480000]
    plan = audio.plan_windows(480000, 16000, downbeats, max_samples=LENGTH)
    assert [p[2] for p in plan] == [5, 5, 2] and plan[0][0] == 8000 and plan[2][1] == int(round(times[-1] * 16000))
    hand = _by_hand(plain, audio.cut_windows(wave[0], plan, LENGTH))
    _assert_windows(result, plan, hand)
    assert [len(w["bars"]) for w in result["windows"]] == [5, 5, 2]
    # a recording shorter than one window: one window, flagged short
    short = transcribe.transcribe_waveform(plain, x[:48000 * 4], sr, hparams=HP)
    assert len(short["windows"]) == 1 and short["windows"][0]["stop_s"] == 4.0 and short["windows"][0]["flags"] == ["short"]
    assert transcribe.transcribe_waveform(plain, x[:0], sr, hparams=HP)["windows"] == []


# ------------------------------------------------------------------------------------------- the module's decoding options
def test_model_options_reach_the_output(dev, plain, rendered):
    from piano_a2s_amd import audio, transcribe
    x = rendered[:, None]
    plan = [(0, LENGTH, 5)]
    w = audio.cut_windows(torch.from_numpy(rendered).to(dev), plan, LENGTH)
    greedy = transcribe.transcribe_waveform(plain, x, 16000, hparams=HP)
    plain.constrained_decoding = True
    constrained = transcribe.transcribe_waveform(plain, x, 16000, hparams=HP)
    assert plain.last_decoded is not None
    _assert_windows(constrained, plan, _by_hand(plain, w))
    plain.constrained_decoding, plain.beam_size = False, 2
    beam = transcribe.transcribe_waveform(plain, x, 16000, hparams=HP)
    assert plain.last_beam_scores is not None
    _assert_windows(beam, plan, _by_hand(plain, w))
    plain.beam_size, plain.alignment = 1, True
    aligned = transcribe.transcribe_waveform(plain, x[LENGTH // 4:], 16000, downbeats=[1.0, 3.0, 5.5, 8.0], hparams=HP)
    assert [b["upper_ids"] for b in aligned["windows"][0]["bars"]] != [] and len(aligned["windows"]) == 1
    win = aligned["windows"][0]
    rec = win["alignment"]
    assert win["start_s"] == 1.0 and win["stop_s"] == 8.0 and win["n_bars"] == 3 and rec["unit"] == "seconds"
    assert len(rec["bar"]) == 3 == len(rec["upper"]) == len(rec["lower"]) == len(rec["bar_weight"])
    seen = 0
    for bar, ids in zip(rec["upper"] + rec["lower"], [b["upper_ids"] for b in win["bars"]] + [b["lower_ids"] for b in win["bars"]]):
        assert len(bar) == len(ids)
        for s in bar:
            if s is not None:
                seen += 1
                assert win["start_s"] <= s <= win["start_s"] + LENGTH / 16000.0
    assert seen > 0 and all(s is None or 1.0 <= s <= 13.0 for s in rec["bar"])
    assert "alignment" not in greedy["windows"][0]
    assert not plain.training


# ------------------------------------------------------------------------------------------- the command line
def test_command_line(tmp_path, state):
    from piano_a2s_amd import audio
    wav = tmp_path / "take one.wav"
    audio.write_wav(wav, _song(44100, 3.0, 2, 2), 44100, bits=16)
    ck_file = tmp_path / "weights.pt"
    torch.save(state, ck_file)
    ck_dir = tmp_path / "CKPT+best"
    ck_dir.mkdir()
    torch.save(state, ck_dir / "transcription.ckpt")
    small = ["--conv_feature_size=32", "--hidden_size=32", "--max_length=(12, 8)"]
    outs = []
    for name, ck, extra in (("a", ck_file, []), ("b", ck_dir, ["--constrained_decoding", "--alignment"])):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "transcribe.py"), os.path.join(ROOT, "hparams", "finetune.yaml"), "--checkpoint", str(ck), str(wav),
                            "--out", str(out)] + extra + small, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        with open(out / "take one.json") as f:
            outs.append(json.load(f))
    for res in outs:
        assert {"sample_rate_in", "sample_rate", "frames_per_second", "windows"} <= set(res)
        assert res["sample_rate_in"] == 44100 and res["sample_rate"] == 16000 and res["frames_per_second"] == 100.0 and len(res["windows"]) == 1
        win = res["windows"][0]
        assert {"start_s", "stop_s", "n_bars", "flags", "time_signature", "key", "bars"} <= set(win)
        assert win["start_s"] == 0.0 and win["stop_s"] == 3.0 and win["n_bars"] == 5 == len(win["bars"])
        assert set(win["bars"][0]) == {"upper", "lower", "upper_ids", "lower_ids"}
    assert "alignment" in outs[1]["windows"][0] and "alignment" not in outs[0]["windows"][0]
