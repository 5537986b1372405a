"""Room acoustics of the rendered synthetic corpus (csrc/a2s_room.hip): every clip's waveform is convolved on the GPU with a
synthetic impulse response of its own -- a direct path, a pre-delay and an exponentially decaying diffuse tail -- between the synthesiser
(piano_a2s_amd.render) and the VQT.

The room is a property of the clip: its parameters are drawn from the clip's own 32-bit seed (`room_seeds`: the noise seed of its render program,
xor 0x524F4F4D), so a clip has the same room in every epoch.  The parameters are computed on the host in float64 and go to the device as one
(B, 4) int32 table [pre, L, wet f32 bits, decay f32 bits]; no integer is derived from fp32 device arithmetic.  There is no CPU implementation of the
signal path in the product (tests/room_oracle.py is the float64 definition the tests compare against)."""
import math

import numpy as np
import torch

from . import hip

ROOM_XOR = 0x524F4F4D
GOLDEN = 0x9E3779B9
STAGES = {"none": (), "train": ("train",), "eval": ("valid", "test"), "all": ("train", "valid", "test")}


def hash32(x):
    """The 32-bit hash of the synthesiser on a uint64 array that holds 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    x = x & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def room_seeds(programs):
    """The room seed of every clip of a batch of render programs (B, 1 + E, 8) int32 ON THE HOST: header word 7 (the noise seed) xor 0x524F4F4D."""
    if torch.is_tensor(programs):
        if programs.is_cuda:
            raise hip.A2SError("room_seeds: takes the programs while they are on the host (nothing is read back from the device)")
        programs = programs.numpy()
    words = np.ascontiguousarray(np.asarray(programs)[:, 0, 7]).astype(np.int32)
    return words.view(np.uint32) ^ np.uint32(ROOM_XOR)


def _range(name, value, lo_min, hi_max):
    if isinstance(value, str):
        value = value.strip().strip("()[]").split(",")
    try:
        lo, hi = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f"--room_{name} must be a range \"(lo, hi)\" of two numbers (got {value!r})") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo_min <= lo <= hi <= hi_max):
        raise ValueError(f"--room_{name} must be a range (lo, hi) with {lo_min} <= lo <= hi <= {hi_max} (got ({lo}, {hi}))")
    return lo, hi


def check_stages(value):
    """--synthetic_room -> one of none | train | eval | all (the default is none); anything else raises ValueError."""
    mode = "none" if value is None else str(value).strip().lower()
    if mode not in STAGES:
        raise ValueError(f"--synthetic_room must be one of none, train, eval, all (got {value!r})")
    return mode


class Room:
    """Per-clip synthetic rooms.  rt60 (seconds), drr_db (direct-to-reverberant ratio) and predelay_ms are ranges (lo, hi); a clip's values are
    lerp(range, v(j)), v(j) = (hash32(seed + j * 0x9E3779B9) >> 8) * 2^-24 for j = 0, 1, 2.  L_max, the longest impulse response, follows from the
    upper ends: rint(predelay_hi * sr / 1000) + ceil(rt60_hi * sr), rounded up to a multiple of 4 (10 000 with the defaults)."""

    def __init__(self, rt60=(0.2, 0.6), drr_db=(0.0, 12.0), predelay_ms=(5.0, 25.0), sample_rate=16000, L_max=None):
        self.sample_rate = int(sample_rate)
        if self.sample_rate < 1000:
            raise ValueError(f"room: the sample rate must be at least 1000 Hz (got {sample_rate!r})")
        self.rt60 = _range("rt60", rt60, 0.01, 10.0)
        self.drr_db = _range("drr_db", drr_db, -40.0, 60.0)
        self.predelay_ms = _range("predelay_ms", predelay_ms, 1.0, 1000.0)
        sr = self.sample_rate
        full = int(np.rint(self.predelay_ms[1] * sr / 1000.0)) + int(math.ceil(self.rt60[1] * sr))
        full = (full + 3) // 4 * 4
        self.L_max = full if L_max is None else int(L_max)          # (a cap below the full length truncates the tails: the tests' short rooms)
        if not 1 <= self.L_max <= full:
            raise ValueError(f"room: L_max must be in 1 .. {full} (got {L_max!r})")
        self.clips = 0                                               # clips processed by apply() so far
        self._buf = {}

    def describe(self):
        return dict(rt60=list(self.rt60), drr_db=list(self.drr_db), predelay_ms=list(self.predelay_ms), sample_rate=self.sample_rate, L_max=self.L_max)

    def draws(self, seeds):
        """seeds (B,) -> (rt60, drr_db, predelay in samples) as float64 / float64 / int64 arrays."""
        s = np.asarray(seeds).astype(np.uint64) & np.uint64(0xFFFFFFFF)
        v = [(hash32(s + np.uint64(j * GOLDEN)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 for j in range(3)]
        lerp = lambda r, t: r[0] + (r[1] - r[0]) * t
        pre = np.rint(lerp(self.predelay_ms, v[2]) * self.sample_rate / 1000.0).astype(np.int64)
        return lerp(self.rt60, v[0]), lerp(self.drr_db, v[1]), np.maximum(pre, 1)

    def params(self, seeds):
        """seeds (B,) of 32-bit values -> the (B, 4) int32 table [pre, L, wet f32 bits, decay f32 bits], in numpy on the host."""
        rt60, drr_db, pre = self.draws(seeds)
        sr = self.sample_rate
        decay = math.log(1000.0) / (rt60 * sr)
        L = np.minimum(self.L_max, pre + np.ceil(rt60 * sr).astype(np.int64))
        wet = 10.0 ** (-drr_db / 20.0) * np.sqrt(3.0 * (1.0 - np.exp(-2.0 * decay)))
        table = np.empty((len(rt60), 4), dtype=np.int32)
        table[:, 0], table[:, 1] = pre, L
        table[:, 2], table[:, 3] = wet.astype(np.float32).view(np.int32), decay.astype(np.float32).view(np.int32)
        return table

    def _buffers(self, device, B, N):
        """The device buffers of a batch shape, made on first use and kept: after the first call of a shape nothing is allocated per step."""
        device = torch.device(device)
        key = (str(device), B, N)
        if key not in self._buf:
            self._buf[key] = dict(host_params=torch.empty((B, 4), dtype=torch.int32), host_seeds=torch.empty((B,), dtype=torch.int32),
                                  params=torch.empty((B, 4), dtype=torch.int32, device=device),
                                  seeds=torch.empty((B,), dtype=torch.int32, device=device),
                                  ir=torch.empty((B, self.L_max), dtype=torch.float32, device=device),
                                  y=torch.empty((B, N), dtype=torch.float32, device=device) if N else None)
        return self._buf[key]

    def _upload(self, seeds, buf):
        seeds = np.asarray(seeds).astype(np.uint64).astype(np.uint32)
        if seeds.shape != (buf["seeds"].shape[0],):
            raise hip.A2SError(f"room: expects one seed per clip ({buf['seeds'].shape[0]}), got an array of shape {seeds.shape}")
        buf["host_params"].numpy()[:] = self.params(seeds)
        buf["host_seeds"].numpy()[:] = seeds.view(np.int32)
        buf["params"].copy_(buf["host_params"])          # (pageable host memory: the copies are staged before they return, the host buffers are free again)
        buf["seeds"].copy_(buf["host_seeds"])

    def _ir(self, seeds, buf):
        self._upload(seeds, buf)
        hip.room_ir(buf["seeds"], buf["params"], self.L_max, ir=buf["ir"])
        return buf["ir"], buf["params"]

    def impulse_responses(self, seeds, device):
        """seeds (B,) -> (ir (B, L_max) float32, params (B, 4) int32), both on the device; the buffers are reused by the next call of this shape."""
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.A2SError("room: the impulse responses are made on the GPU only (no CPU implementation in the product)")
        return self._ir(seeds, self._buffers(device, len(seeds), 0))

    def apply(self, wave, seeds):
        """wave (B, N) float32 on the device, seeds (B,) -> the reverberant waveforms (B, N): y[n] = sum_k h[k] wave[n - k], not rescaled
        (|y| <= sum|h| * max|wave|; the VQT normalises per clip).  The result lives in a buffer that the next call of this shape overwrites."""
        if not torch.is_tensor(wave) or not wave.is_cuda:
            raise hip.A2SError("room.apply runs on the GPU only (no CPU implementation in the product)")
        if wave.dim() != 2 or wave.dtype != torch.float32:
            raise hip.A2SError("room.apply: expects (B, N) float32 waveforms")
        B, N = wave.shape
        if B == 0 or N == 0:
            return wave
        buf = self._buffers(wave.device, B, N)
        ir, params = self._ir(seeds, buf)
        hip.fir_rows(wave if wave.stride(1) == 1 else wave.contiguous(), ir, params, self.L_max, y=buf["y"])
        self.clips += B
        return buf["y"]
