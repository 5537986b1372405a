"""Float64 numpy restatement of the synthesiser's signal definition (the device kernel is csrc/a2s_render.hip).

One program = (1 + E, 8) int32: row 0 the header [n_samples, n_rows, attack, rel_len, rel_rate f32, gain f32, noise_level f32, noise_seed u32], rows
1 .. E the notes [onset, length, inc1 u32, amp f32, decay f32, g f32, n_harm, 0].  A row with length <= 0, onset >= n_samples (or onset < 0) is padding.

    wave[n] = gain * sum_rows amp * env(m) * sum_{h = 1 .. n_harm, h * inc1 < 2^31} g^(h-1) * sin(2 pi x_h(m))  +  noise_level * u(n)
    m       = n - onset, the row contributes for 0 <= m < length + rel_len
    x_h(m)  = ((uint32)(m * h * inc1) >> 8) * 2^-24
    env(m)  = min(1, (m + 1) / attack) * exp(-m * decay) * (m >= length ? exp(-(m - length) * rel_rate) : 1)
    u(n)    = (hash32(noise_seed + n * 0x9E3779B9) >> 8) * 2^-23 - 1

Everything but the integer phase and the hash is evaluated in float64 from the float32 values the program holds."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def hash32(x):
    """x: uint64 array holding 32-bit values."""
    x = x & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def noise_unit(seed, n):
    """u(n) for sample indices n (integer array): exact in float64 (and in float32)."""
    n = np.asarray(n, dtype=np.uint64)
    h = hash32(np.uint64(seed) + n * np.uint64(0x9E3779B9))
    return (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0


def _f32(word):
    return float(np.array(word, dtype=np.int32).view(np.float32))


def header(program):
    h = program[0]
    return dict(n_samples=int(h[0]), n_rows=int(h[1]), attack=int(h[2]), rel_len=int(h[3]), rel_rate=_f32(h[4]), gain=_f32(h[5]),
                noise_level=_f32(h[6]), noise_seed=int(np.array(h[7], dtype=np.int32).view(np.uint32)))


def live_rows(program):
    """Indices (1-based) of the rows that are not padding, ascending."""
    hd = header(program)
    last = min(hd["n_rows"], program.shape[0] - 1)
    return [i for i in range(1, last + 1) if program[i, 1] > 0 and 0 <= program[i, 0] < hd["n_samples"]]


def render(program, n_samples=None):
    """(1 + E, 8) int32 -> (n_samples,) float64."""
    program = np.asarray(program, dtype=np.int32)
    hd = header(program)
    N = hd["n_samples"] if n_samples is None else n_samples
    acc = np.zeros(N, dtype=np.float64)
    attack = max(1, hd["attack"])
    for i in live_rows(program):
        onset, length = int(program[i, 0]), int(program[i, 1])
        inc = int(np.array(program[i, 2], dtype=np.int32).view(np.uint32))
        amp, decay, g = _f32(program[i, 3]), _f32(program[i, 4]), _f32(program[i, 5])
        n_harm = min(int(program[i, 6]), 16)
        end = min(min(N, hd["n_samples"]), onset + length + hd["rel_len"])
        if end <= onset:
            continue
        m = np.arange(end - onset, dtype=np.int64)
        env = np.minimum(1.0, (m + 1) / attack) * np.exp(-m * decay)
        env = env * np.where(m >= length, np.exp(-(m - length) * hd["rel_rate"]), 1.0)
        tone = np.zeros(len(m), dtype=np.float64)
        for h in range(1, n_harm + 1):
            if h * inc >= 2 ** 31:
                break
            phase = (m.astype(np.uint64) * np.uint64(h * inc)) & M32
            x = (phase >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
            tone += g ** (h - 1) * np.sin(2.0 * np.pi * x)
        acc[onset:end] += amp * env * tone
    out = hd["gain"] * acc
    if hd["noise_level"] != 0.0:
        live = min(N, hd["n_samples"])
        out[:live] += hd["noise_level"] * noise_unit(hd["noise_seed"], np.arange(live))
    return out


def isolated_events(events, rel_len=1600, min_length=1600, semitones=2.0):
    """The events (n, 3) [onset, length, midi] that last at least `min_length` samples and that no other event overlaps -- sounding, its release
    included, at some time of the event -- within `semitones` of the pitch with its fundamental or with its second or third partial."""
    out = []
    for i, (onset, length, midi) in enumerate(events):
        if length < min_length:
            continue
        clear = True
        for j, (o, l, m) in enumerate(events):
            if j == i or o >= onset + length or o + l + rel_len <= onset:
                continue
            if min(abs(m + 12.0 * np.log2(h) - midi) for h in (1, 2, 3)) <= semitones:
                clear = False
                break
        if clear:
            out.append((int(onset), int(length), int(midi)))
    return out
