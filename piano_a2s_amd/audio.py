"""From an audio file to the 16 kHz mono waveforms the GPU VQT takes.

The reference reads its recordings with ``librosa.load(path, sr=16000)`` (reference utilities.py, get_VQT): decode, mix to mono, resample with libsoxr.
This module restates that layer: `read_wav` decodes RIFF/WAVE files on the host, `Resampler` mixes and resamples on the GPU (csrc/a2s_resample.hip, a
rational polyphase filter) with a Kaiser-windowed sinc of the SAME convention as the VQT's decimator (vqt.decimation_filter), `plan_windows` and
`cut_windows` cut a recording into the clips the model takes.  soxr's coefficients are not published, so parity with the reference's waveforms stays
unpinned -- the caveat of the VQT decimator.  Host side: numpy and torch only."""
import math
import struct

import numpy as np
import torch

from . import hip


# ------------------------------------------------------------------------------------------- filter
def resample_filter(sr_in, sr_out=16000, passband=0.913, atten_db=120.0):
    """The polyphase table of the conversion sr_in -> sr_out: (table float32 (L, K), L, M, K, Hh) with L / M = sr_out / sr_in in lowest terms and
    table[p][i] = h[p + (i - Hh) L], h the Kaiser-windowed sinc at the rate sr_in * L (taps h[-half .. half], normalised to sum L; band edges relative to
    the lower of the two Nyquist frequencies: passband 0.913, stop band from 1.0, as vqt.decimation_filter).  sr_in == sr_out: the identity, K = 1."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample_filter: sample rates must be positive (got {sr_in}, {sr_out})")
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    if L == M:
        return np.ones((1, 1), dtype=np.float32), 1, 1, 1, 0
    h, half = _prototype(sr_in, sr_out, L, passband, atten_db)
    Hh = -(-half // L)
    K = 2 * Hh + 1
    t = np.arange(L)[:, None] + (np.arange(K)[None, :] - Hh) * L          # position in h, relative to its centre
    inside = np.abs(t) <= half
    table = np.where(inside, h[np.clip(t + half, 0, 2 * half)], 0.0)
    return np.ascontiguousarray(table, dtype=np.float32), L, M, K, Hh


def _prototype(sr_in, sr_out, L, passband, atten_db):
    ratio = (min(sr_in, sr_out) / 2.0) / (sr_in * L)                      # the lower Nyquist frequency at the rate sr_in * L
    width = (1.0 - passband) * ratio
    cutoff = (1.0 + passband) / 2.0 * ratio
    half = int(math.ceil((atten_db - 8.0) / (2.285 * 2.0 * math.pi * width) / 2.0))
    n = np.arange(-half, half + 1)
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * n) * np.kaiser(2 * half + 1, 0.1102 * (atten_db - 8.7))
    return h / h.sum() * L, half


def resample_prototype(sr_in, sr_out=16000, passband=0.913, atten_db=120.0):
    """(h float64 (2 half + 1,), half): the prototype low-pass resample_filter cuts into phases."""
    g = math.gcd(int(sr_in), int(sr_out))
    return _prototype(int(sr_in), int(sr_out), int(sr_out) // g, passband, atten_db)


class Resampler:
    """Mono mix and sample-rate conversion on the GPU: (x (B, N, C) or (B, N) float32, n_in=None) -> (y (B, n_out_max) float32, n_out (B,) int64).
    n_in: frames per clip (a sequence or an int32 / int64 tensor), default N for every clip; y is zero at and behind n_out[b] = ceil(n_in[b] L / M).
    The table lives on the device.  sr_in == sr_out with one channel returns its input; with more channels the kernel still runs, with the identity
    table, so that there is one mono mix."""

    def __init__(self, device, sr_in, sr_out=16000):
        self.device = torch.device(device)
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        table, self.L, self.M, self.K, self.Hh = resample_filter(sr_in, sr_out)
        self.table = torch.from_numpy(table).to(self.device)

    def n_out(self, n_in):
        return -(-int(n_in) * self.L // self.M)

    def __call__(self, x, n_in=None):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise hip.A2SError("Resampler runs on the GPU only (no CPU implementation in the product)")
        if x.dim() not in (2, 3) or x.dtype != torch.float32:
            raise hip.A2SError(f"Resampler: x must be a float32 tensor (B, N) or (B, N, C) (got {tuple(x.shape)}, {x.dtype})")
        B, N = x.shape[:2]
        C = x.shape[2] if x.dim() == 3 else 1
        if n_in is None:
            n_in = torch.full((B,), N, dtype=torch.int32, device=x.device)
        else:
            n_in = torch.as_tensor(n_in, device=x.device).to(torch.int32).reshape(B).clamp(0, N)
        n_out = (n_in.to(torch.int64) * self.L + (self.M - 1)) // self.M
        if self.L == self.M and C == 1:
            return x.reshape(B, N), n_out
        n_out_max = self.n_out(N)
        if B == 0 or n_out_max == 0:
            return torch.zeros((B, n_out_max), dtype=torch.float32, device=x.device), n_out
        y = hip.resample_rows(x.contiguous().reshape(B, N * C), n_in.contiguous(), self.table, self.M, self.Hh, channels=C, n_out_max=n_out_max, n_in_max=N)
        return y, n_out


# ------------------------------------------------------------------------------------------- WAV files
_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def read_wav(path):
    """A RIFF/WAVE file -> (float32 array (frames, channels), sample_rate).  PCM (format 1) at 8 (unsigned), 16, 24 and 32 bits, scaled by
    2^-(bits - 1); IEEE float (format 3) at 32 and 64 bits; WAVE_FORMAT_EXTENSIBLE (0xFFFE) through the first two bytes of its sub-format.  Chunks are
    walked with their pad bytes, unknown ones skipped; a data chunk that claims more than the file holds is cut to whole frames.  Anything else
    raises ValueError naming the format code."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(blob):
        cid, size = struct.unpack_from("<4sI", blob, pos)
        body = pos + 8
        if cid == b"fmt ":
            if size < 16 or body + 16 > len(blob):
                raise ValueError(f"{path}: short fmt chunk ({size} bytes)")
            code, channels, rate, _, block, bits = struct.unpack_from("<HHIIHH", blob, body)
            if code == _EXTENSIBLE:
                if size < 40 or body + 40 > len(blob):
                    raise ValueError(f"{path}: format 0xFFFE (extensible) with a fmt chunk of {size} bytes, too short for a sub-format")
                code = struct.unpack_from("<H", blob, body + 24)[0]
            fmt = (code, channels, rate, block, bits)
        elif cid == b"data":
            data = blob[body:body + size]                                  # (a slice ends at the end of the file)
            break
        pos = body + size + (size & 1)
    if fmt is None:
        raise ValueError(f"{path}: no fmt chunk before the data")
    if data is None:
        raise ValueError(f"{path}: no data chunk")
    code, channels, rate, block, bits = fmt
    if channels < 1:
        raise ValueError(f"{path}: format {code} with {channels} channels")
    if (code, bits) not in ((_PCM, 8), (_PCM, 16), (_PCM, 24), (_PCM, 32), (_FLOAT, 32), (_FLOAT, 64)):
        raise ValueError(f"{path}: unsupported WAVE format code {code} (0x{code:04X}) at {bits} bits: PCM (1) at 8, 16, 24, 32 bits and IEEE float (3) at 32, 64 "
                         "bits are read")
    width = bits // 8
    frames = len(data) // (width * channels)
    data = data[:frames * width * channels]
    if code == _FLOAT:
        x = np.frombuffer(data, dtype="<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 8:
        x = (np.frombuffer(data, dtype=np.uint8).astype(np.float32) - 128.0) * 2.0 ** -7
    elif bits == 24:
        b = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = ((v ^ 0x800000) - 0x800000).astype(np.float64) * 2.0 ** -23
    else:
        x = np.frombuffer(data, dtype="<i2" if bits == 16 else "<i4").astype(np.float64) * 2.0 ** -(bits - 1)
    return np.ascontiguousarray(x.reshape(frames, channels), dtype=np.float32), int(rate)


def quantise(x, bits=16):
    """The integers write_wav stores for the samples x: round(x 2^(bits - 1)), clipped to the format's range."""
    full = 2.0 ** (bits - 1)
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * full), -full, full - 1).astype(np.int64)


def write_wav(path, x, sr, bits=16):
    """x (frames,) or (frames, channels) in [-1, 1) -> a PCM file at 8 (unsigned), 16, 24 or 32 bits; bits = -32: IEEE float32."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError(f"write_wav: x must be (frames,) or (frames, channels) (got {x.shape})")
    if bits == -32:
        code, width, payload = _FLOAT, 4, x.astype("<f4").tobytes()
    elif bits in (8, 16, 24, 32):
        code, width, q = _PCM, bits // 8, quantise(x, bits)
        if bits == 8:
            payload = (q + 128).astype(np.uint8).tobytes()
        elif bits == 24:
            payload = (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        else:
            payload = q.astype("<i2" if bits == 16 else "<i4").tobytes()
    else:
        raise ValueError(f"write_wav: bits must be 8, 16, 24, 32 or -32 (float32) (got {bits})")
    channels = x.shape[1]
    fmt = struct.pack("<HHIIHH", code, channels, int(sr), int(sr) * channels * width, channels * width, 8 * width)
    pad = b"\0" if len(payload) & 1 else b""
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload + pad
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


MIDI_TICKS_PER_QUARTER = 500
MIDI_TEMPO_US = 500000          # per quarter: with 500 ticks per quarter one tick is one millisecond


def _vlq(n):
    """A MIDI variable-length quantity: 7 bits per byte, most significant first, the top bit set on every byte but the last."""
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append(0x80 | (n & 0x7F))
        n >>= 7
    return bytes(reversed(out))


def midi_bytes(notes, velocity=64):
    """notes [[onset_s, length_s, midi]] or [[onset_s, length_s, midi, velocity]] -> a Standard MIDI File, format 0: one track on channel 0,
    MIDI_TICKS_PER_QUARTER ticks per quarter at MIDI_TEMPO_US microseconds per quarter, so a tick is 1 ms; a note without a velocity of its own (or
    with None) gets `velocity`.  Onset and end are rounded to ticks and a note lasts at least one; at equal times the note-offs come first, then by
    pitch.  Onsets before 0, pitches outside 0 .. 127 and velocities outside 1 .. 127 are ValueErrors."""
    events = []
    for onset, length, midi, *own in notes:
        given = bool(own) and own[0] is not None
        vel = own[0] if given else velocity
        on = int(round(float(onset) * 1e6 * MIDI_TICKS_PER_QUARTER / MIDI_TEMPO_US))
        off = max(on + 1, int(round((float(onset) + float(length)) * 1e6 * MIDI_TICKS_PER_QUARTER / MIDI_TEMPO_US)))
        if on < 0 or not 0 <= int(midi) <= 127 or int(midi) != midi:
            raise ValueError(f"write_midi: not a note: onset {onset!r} s, pitch {midi!r}")
        if len(own) > 1 or (given and (int(vel) != vel or not 1 <= int(vel) <= 127)):
            raise ValueError(f"write_midi: not a velocity in 1 .. 127: {own!r}")
        events += [(on, 1, int(midi), int(vel)), (off, 0, int(midi), int(vel))]
    events.sort()
    track, now = b"\x00\xff\x51\x03" + MIDI_TEMPO_US.to_bytes(3, "big"), 0
    for tick, is_on, midi, vel in events:
        track += _vlq(tick - now) + bytes([0x90 if is_on else 0x80, midi, vel])
        now = tick
    track += b"\x00\xff\x2f\x00"
    return b"MThd" + struct.pack(">IHHH", 6, 0, 1, MIDI_TICKS_PER_QUARTER) + b"MTrk" + struct.pack(">I", len(track)) + track


def write_midi(path, notes, velocity=64):
    """midi_bytes(notes) to a file.  notes: [[onset_s, length_s, midi]] or [[onset_s, length_s, midi, velocity]], or a result of transcribe_waveform
    (result_notes)."""
    if not 1 <= int(velocity) <= 127:
        raise ValueError(f"write_midi: velocity must be in 1 .. 127 (got {velocity!r})")
    data = midi_bytes(result_notes(notes) if isinstance(notes, dict) else notes, velocity)
    with open(path, "wb") as f:
        f.write(data)


def result_notes(result):
    """The notes of a transcription result in recording time: every bar's "retimed" where it has one (performed_timing), else its "performed" (align_notes), its "notes" otherwise
    (resynthesis); bars without either give nothing.  A bar with "dynamics" gives every note its velocity as a fourth entry (where it has one), and
    the notes a bar marks in "quiet" are left out."""
    out = []
    for win in result.get("windows", []):
        for bar in win.get("bars", []):
            notes = [list(n) for n in bar.get("retimed", bar.get("performed", bar.get("notes", [])))]
            if "dynamics" in bar:
                notes = [n + [d[1]] if d[1] is not None else n for n, d in zip(notes, bar["dynamics"])]
            out += [n for n, q in zip(notes, bar.get("quiet", [False] * len(notes))) if not q]
    return out


# ------------------------------------------------------------------------------------------- windows
def plan_windows(n_samples, sr=16000, downbeats=None, window_seconds=12.0, hop_seconds=None, max_bars=5, max_samples=None):
    """The clips a recording of n_samples is cut into: [(start, stop, n_bars)] in samples, each at most min(window_seconds * sr, max_samples) long
    (max_samples: (max_frame_num - 1) * hop_length of the hparams; default 12 s).
    With downbeats (seconds, ascending): consecutive bars in groups of max_bars, not overlapping (the reference's test protocol: ProcessASAP cuts
    downbeats[i] .. downbeats[i + max_bars]).  A group longer than the window keeps as many leading bars as fit, at least one; a single bar longer than
    the window is cut at the window (plan_flags marks it); the next group starts at the first bar not kept.  Nothing before the first and behind the
    last downbeat is transcribed.  Without downbeats: windows every hop_seconds (default: the window), n_bars = max_bars, the last one may be short."""
    return [w[:3] for w in _plan(n_samples, sr, downbeats, window_seconds, hop_seconds, max_bars, max_samples)]


def plan_flags(n_samples, sr=16000, downbeats=None, window_seconds=12.0, hop_seconds=None, max_bars=5, max_samples=None):
    """Per window of plan_windows its list of flags: "bar_cut" (one bar longer than the window, cut at the window), "short" (no downbeats: the
    recording ends inside the window)."""
    return [w[3] for w in _plan(n_samples, sr, downbeats, window_seconds, hop_seconds, max_bars, max_samples)]


def plan_bar_lines(n_samples, sr=16000, downbeats=None, window_seconds=12.0, hop_seconds=None, max_bars=5, max_samples=None):
    """Per window of plan_windows its n_bars + 1 bar lines, in samples from the window's start: strictly ascending, the first 0, the last stop - start
    (for a "bar_cut" window: [0, the window's length], the one bar ends where the window does).  Without downbeats the bars have no position: None per
    window."""
    return [w[4] for w in _plan(n_samples, sr, downbeats, window_seconds, hop_seconds, max_bars, max_samples)]


def _plan(n_samples, sr, downbeats, window_seconds, hop_seconds, max_bars, max_samples):
    n_samples, max_bars = int(n_samples), int(max_bars)
    limit = min(int(round(float(window_seconds) * sr)), int(max_samples) if max_samples is not None else 12 * int(sr))
    if limit < 1 or max_bars < 1:
        raise ValueError(f"plan_windows: needs a window of at least one sample and max_bars >= 1 (got {window_seconds} s at {sr} Hz, max_bars = {max_bars})")
    out = []
    if downbeats is None:
        hop = limit if hop_seconds is None else int(round(float(hop_seconds) * sr))
        if hop < 1:
            raise ValueError(f"plan_windows: hop_seconds must give at least one sample (got {hop_seconds})")
        start = 0
        while start < n_samples:
            stop = min(start + limit, n_samples)
            out.append((start, stop, max_bars, ["short"] if stop - start < limit else [], None))
            if stop == n_samples:
                break
            start += hop
        return out
    db = [int(round(float(t) * sr)) for t in downbeats]
    if any(b < a for a, b in zip(db, db[1:])):
        raise ValueError("plan_windows: downbeats must ascend")
    db = [min(max(t, 0), n_samples) for t in db]
    i = 0
    while i + 1 < len(db):
        if db[i + 1] <= db[i]:                                              # (an empty bar: behind the end of the recording, or a repeated time)
            i += 1
            continue
        keep = 1
        while keep < max_bars and i + keep + 1 < len(db) and db[i + keep + 1] > db[i + keep] and db[i + keep + 1] - db[i] <= limit:
            keep += 1
        stop, flags = db[i + keep], []
        if stop - db[i] > limit:                                            # (keep == 1: one bar longer than the window)
            stop, flags = db[i] + limit, ["bar_cut"]
        lines = [t - db[i] for t in db[i:i + keep]] + [stop - db[i]]        # (ascending: the loop above keeps non-empty bars only)
        out.append((db[i], stop, keep, flags, lines))
        i += keep
    return out


def cut_windows(wave16k, plan, length):
    """wave16k (N,) float32 on the device and a plan of plan_windows -> (W, length) float32 on the device: window w holds wave16k[start:stop], zeros
    behind it."""
    if not torch.is_tensor(wave16k) or wave16k.dim() != 1:
        raise ValueError("cut_windows: wave16k must be a 1-D tensor")
    out = torch.zeros((len(plan), int(length)), dtype=torch.float32, device=wave16k.device)
    for w, (start, stop, *_) in enumerate(plan):
        if stop - start > length:
            raise ValueError(f"cut_windows: window {w} has {stop - start} samples, more than {length}")
        out[w, :stop - start] = wave16k[start:stop]
    return out
