"""Augmentation of a training batch on the device: transposition, tempo (section 18) and the spectrogram's colour, noise floor and
masks (section 20, at the end of this file).

Transposition: per clip a whole number of semitones s and a detuning of
delta feature bins are drawn on the host; csrc/a2s_augment.hip respells the targets (kern_transpose's tables) and shifts the feature rows by
bins_per_semitone * s + delta bins.  A clip whose score cannot be respelled keeps its score and key and is only detuned.

The draws come from the object's own numpy Generator: Python's `random`, numpy's global state and torch's generators never advance (the
teacher-forcing draw protocol of the training step depends on them)."""
import numpy as np
import torch

from piano_a2s_amd import kern_transpose
from piano_a2s_amd.abi import A2SError

MAX_SEMITONES = kern_transpose.MAX_SEMITONES
MAX_DETUNE_BINS = 2.5
MAX_TEMPO_CHANGE = 0.25
_TEMPO_STREAM = 0x74656D70          # "temp": what sets the tempo generator's seed sequence apart from the transposer's


class _Augment:
    """What the three augmenters share.  Each class states what the recipe needs to wire it (recipe.AUGMENTERS): `flags`, its switches with their
    defaults; `needs`, how a refusal names them; `read`, the constructor's settings from a run's hparams; `cache`, the attribute of the Brain that keeps
    the augmenter; `summary`, its block in run_summary.json and `settings()` what the block states beside the counts; `stats`, the names of its counts in
    the train stats; `rewrites_targets`, whether the targets of a batch change in place."""
    flags, needs, cache, summary = (), None, None, None
    count_names, stats = (), ()
    rewrites_targets = False
    _stream = ()          # what sets the class's seed sequence apart from the others'

    def __init__(self, cfg, seed, device, rank):
        self.freq_bins = int(cfg["freq_bins"])
        self.seed, self.rank = int(seed), int(rank)
        self.device = torch.device(device)
        self._rng = None
        self._counters = None
        self.last_plan = None
        self.reseed(0, self.rank)

    @classmethod
    def _flag_values(cls, hparams):
        return [getattr(hparams, flag, default) for flag, default in cls.flags]

    # ------------------------------------------------------------------ host side
    def reseed(self, epoch, rank=None):
        """The draws that follow are a function of (seed, rank, epoch) alone."""
        if rank is not None:
            self.rank = int(rank)
        self._rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([self.seed & 0xFFFFFFFFFFFFFFFF, self.rank, int(epoch or 0), *self._stream])))

    # ------------------------------------------------------------------ device side
    def _features(self, batch):
        """(the batch as a list, its features), or A2SError where they are not (B, 1, T, freq_bins)."""
        batch = list(batch)
        x = batch[0]
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[-1] != self.freq_bins:
            raise A2SError(f"{type(self).__name__}: expects features (B, 1, T, {self.freq_bins}), got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        return batch, x

    def _stage(self, array, dtype):
        """A host array on the device: pinned staging from the caching host allocator, which keeps a block until the copy that reads it has run."""
        return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype)).pin_memory().to(self.device, non_blocking=True)

    def _count_tensor(self):
        if self._counters is None:
            self._counters = torch.zeros(len(self.count_names), dtype=torch.int32, device=self.device)
        return self._counters

    def __call__(self, batch):
        draws = self.draw(batch[0].shape[0])
        return self.apply(batch, *(draws if isinstance(draws, tuple) else (draws,)))

    def counts(self):
        """{name: count so far} over `count_names`: one device-to-host copy."""
        return dict(zip(self.count_names, [0] * len(self.count_names) if self._counters is None else self._counters.tolist()))


def check_range(max_semitones, detune_bins):
    """(K, D) as numbers, or ValueError: K a whole number in 0 .. 6, 0 <= D <= 2.5."""
    try:
        K, D = int(max_semitones), float(detune_bins)
        whole = K == float(max_semitones)
    except (TypeError, ValueError):
        raise ValueError(f"--transpose_augment / --detune_bins must be numbers (got {max_semitones!r}, {detune_bins!r})") from None
    if not whole or not 0 <= K <= MAX_SEMITONES:
        raise ValueError(f"--transpose_augment must be a whole number in 0 .. {MAX_SEMITONES} (got {max_semitones!r})")
    if not 0.0 <= D <= MAX_DETUNE_BINS:
        raise ValueError(f"--detune_bins must be in 0 .. {MAX_DETUNE_BINS} (got {detune_bins!r})")
    return K, D


class TransposeAugment(_Augment):
    """cfg: the transcription module's configuration (freq_bins); max_semitones K in 0 .. 6 and detune_bins D in [0, 2.5]: s uniform in -K .. K,
    delta uniform in [-D, D] per clip; seed: the run's; device: where the batches live.  bins_per_octave: the features' resolution."""

    flags, needs = (("transpose_augment", 0), ("detune_bins", 0.0)), "--transpose_augment needs"
    cache, summary = "_augment", "transpose_augment"
    count_names, stats = ("clips", "transposed", "not_representable"), ("augmented_clips", "transposed_clips", "not_representable_clips")
    rewrites_targets = True

    @classmethod
    def read(cls, hparams):
        """The constructor's settings as the run's hparams state them, or None when both switches are 0; ValueError where one is out of range."""
        K, D = check_range(*cls._flag_values(hparams))
        return dict(max_semitones=K, detune_bins=D, bins_per_octave=getattr(hparams, "bins_per_octave", 60)) if K or D else None

    def settings(self):
        return dict(max_semitones=self.K, detune_bins=self.D)

    def __init__(self, cfg, max_semitones, detune_bins, seed, device, bins_per_octave=60, rank=0):
        self.K, self.D = check_range(max_semitones, detune_bins)
        bpo = int(bins_per_octave)
        if bpo != bins_per_octave or bpo < 12 or bpo % 12:
            raise ValueError(f"transposition augmentation needs a whole number of feature bins per semitone: bins_per_octave = {bins_per_octave!r} is no multiple of 12")
        self.bins_per_semitone = bpo // 12
        super().__init__(cfg, seed, device, rank)
        if self.freq_bins < bpo or self.freq_bins % self.bins_per_semitone:
            raise ValueError(f"transposition augmentation: freq_bins = {self.freq_bins} is not a whole number of semitones of {self.bins_per_semitone} bins "
                             f"spanning at least one octave")
        self._tables = None

    def draw(self, B):
        """(semitones (B,) int32, detune (B,) float32) of the next batch; host only."""
        s = self._rng.integers(-self.K, self.K + 1, size=B).astype(np.int32)
        d = self._rng.uniform(-self.D, self.D, size=B).astype(np.float32) if self.D > 0 else np.zeros(B, dtype=np.float32)
        return s, d

    def apply(self, batch, semitones, detune):
        """The batch (features (B, 1, T, F) float32, ts, key (B, bars), upper (B, bars, U), upper lengths, lower (B, bars, L), ... on the device) under
        the given draws: two launches on the current stream.  Returns the batch with a NEW feature tensor; key, upper and lower are the same tensors,
        rewritten in place."""
        from piano_a2s_amd import hip
        batch, x = self._features(batch)
        key, upper, lower = batch[2], batch[3], batch[5]
        B = x.shape[0]
        if len(semitones) != B or len(detune) != B:
            raise A2SError(f"TransposeAugment: {len(semitones)} / {len(detune)} draws for {B} clips")
        if self._tables is None:
            self._tables = tuple(torch.from_numpy(np.array(t)).to(self.device) for t in kern_transpose.tables())
        eff = torch.empty(B, dtype=torch.float32, device=self.device)
        hip.transpose_targets(*self._tables, self._stage(semitones, np.int32), self._stage(detune, np.float32), key, upper, lower, self.bins_per_semitone, eff,
                              self._count_tensor())
        batch[0] = hip.shift_bins(x.contiguous(), eff)          # one fresh tensor per batch, as the un-augmented path's input is
        return batch


def check_tempo(max_change):
    """R as a float, or ValueError: the largest relative change of the durations, 0 <= R <= 0.25."""
    try:
        R = float(max_change)
    except (TypeError, ValueError):
        raise ValueError(f"--tempo_augment must be a number (got {max_change!r})") from None
    if not 0.0 <= R <= MAX_TEMPO_CHANGE:          # (also a NaN)
        raise ValueError(f"--tempo_augment must be in 0 .. {MAX_TEMPO_CHANGE} (got {max_change!r})")
    return R


class TempoAugment(_Augment):
    """Tempo augmentation: every clip of a batch is played c times as slowly, c uniform in [1 - R, 1 + R] narrowed per clip so
    that its content still lasts at least `min_frames` frames and still ends inside the window -- the reference's MIDIProcess.ramdom_scaling with
    frames for seconds.  The features are resampled along time by csrc/a2s_tempo.hip; no target changes (a **kern score does not state a tempo).

    cfg: the transcription module's configuration (freq_bins); R in [0, 0.25]; seed: the run's; device: where the batches live.  The host draws one
    u in [0, 1) per clip from the object's own Generator (seeded from (seed, rank, epoch) and a constant, so that its stream is not the transposer's);
    where a clip's content ends, which interval is feasible and the factor itself are found on the device: nothing is read back."""

    flags, needs = (("tempo_augment", 0.0),), "--tempo_augment needs"
    cache, summary = "_tempo", "tempo_augment"
    count_names, stats = ("clips", "stretched", "kept"), ("tempo_clips", "tempo_stretched_clips", "tempo_kept_clips")
    _stream = (_TEMPO_STREAM,)

    @classmethod
    def read(cls, hparams):
        """The constructor's settings as the run's hparams state them, or None when R is 0; ValueError where it is out of range."""
        R = check_tempo(*cls._flag_values(hparams))
        return dict(R=R) if R else None

    def settings(self):
        return dict(max_change=self.R)

    def __init__(self, cfg, R, seed, device, rank=0, min_frames=400):
        self.R = check_tempo(R)
        super().__init__(cfg, seed, device, rank)
        self.min_frames = int(min_frames)
        if self.min_frames < 1:
            raise ValueError(f"tempo augmentation: min_frames must be >= 1 (got {min_frames!r})")

    def draw(self, B):
        """u (B,) float32 in [0, 1) of the next batch; host only."""
        return self._rng.random(size=B, dtype=np.float32)

    def apply(self, batch, u):
        """The batch (features (B, 1, T, F) float32 on the device first) under the given draws: two launches on the current stream.  Returns the batch
        with a NEW feature tensor; everything else is the same objects, untouched."""
        from piano_a2s_amd import hip
        batch, x = self._features(batch)
        B, rows = x.shape[0], x.shape[1] * x.shape[2]
        if len(u) != B:
            raise A2SError(f"TempoAugment: {len(u)} draws for {B} clips")
        u_dev = self._stage(u, np.float32)
        content = torch.empty(B, dtype=torch.int32, device=self.device)
        step = torch.empty(B, dtype=torch.int32, device=self.device)
        x = x.contiguous()
        hip.tempo_plan(x, u_dev, self.R, max(1, min(self.min_frames, rows // 3)), content, step, self._count_tensor())      # (short test windows still get stretched)
        batch[0] = hip.stretch_frames(x, step)          # one fresh tensor per batch, as the un-augmented path's input is
        self.last_plan = (content, step)                # (device tensors; reading them synchronises -- tests and tools only)
        return batch


MAX_EQ_DB = 12.0
NOISE_DB_RANGE = (20.0, 80.0)
MAX_MASK_TIME, MAX_MASK_FREQ, MAX_MASKS = 100, 60, 4
NOISE_TILT_DB_PER_OCTAVE = 3.0
_SPECAUG_STREAM = 0x73706563          # "spec": the third augmenter's seed sequence is neither the transposer's nor the tempo generator's


def _whole(flag, value, lo, hi):
    try:
        n = int(value)
        ok = n == float(value)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"--{flag} must be a whole number (got {value!r})") from None
    if not ok or not lo <= n <= hi:
        raise ValueError(f"--{flag} must be a whole number in {lo} .. {hi} (got {value!r})")
    return n


def check_specaug(eq_db=0.0, noise_db=None, mask_time=0, mask_freq=0, mask_count=2):
    """(E, (lo, hi) or None, Wt, Wf, m) as numbers, or ValueError naming the flag: 0 <= E <= 12 dB; the noise floor lo .. hi dB below the clip's peak,
    20 <= lo <= hi <= 80 (a string "(lo, hi)" or two numbers; None: off); Wt in 0 .. 100 frames; Wf in 0 .. 60 bins; m in 1 .. 4."""
    try:
        E = float(eq_db)
    except (TypeError, ValueError):
        raise ValueError(f"--eq_augment_db must be a number (got {eq_db!r})") from None
    if not 0.0 <= E <= MAX_EQ_DB:          # (also a NaN)
        raise ValueError(f"--eq_augment_db must be in 0 .. {MAX_EQ_DB} (got {eq_db!r})")
    noise = None
    if noise_db is not None:
        value = noise_db.strip().strip("()[]").split(",") if isinstance(noise_db, str) else noise_db
        try:
            lo, hi = (float(v) for v in value)
        except (TypeError, ValueError):
            raise ValueError(f"--noise_augment_db must be a range \"(lo, hi)\" of two numbers (got {noise_db!r})") from None
        if not NOISE_DB_RANGE[0] <= lo <= hi <= NOISE_DB_RANGE[1]:
            raise ValueError(f"--noise_augment_db must be a range (lo, hi) with {NOISE_DB_RANGE[0]} <= lo <= hi <= {NOISE_DB_RANGE[1]} (got ({lo}, {hi}))")
        noise = (lo, hi)
    return E, noise, _whole("mask_time", mask_time, 0, MAX_MASK_TIME), _whole("mask_freq", mask_freq, 0, MAX_MASK_FREQ), _whole("mask_count", mask_count, 1, MAX_MASKS)


def specaug_table(F, e, phi, level_db, tilt, bins_per_octave, eq=True, noise=True):
    """One clip's table (2, F) float32 from its draws, formed in float64 (tests/specaug_oracle.py restates it): row 0 the power
    gains G_k = 10^(g_k / 10), g_k = e0 (2z - 1) + e1 cos 2 pi (z + phi1) + e2 cos 2 pi (2z + phi2) dB with z = k / (F - 1); row 1 the noise powers
    v_k = 10^((-level_db + tilt (k - (F - 1) / 2) / bins_per_octave) / 10).  eq / noise False: G = 1 / v = 0."""
    k = np.arange(F, dtype=np.float64)
    z = k / (F - 1) if F > 1 else np.full(1, 0.5)
    out = np.empty((2, F), dtype=np.float64)
    g = e[0] * (2.0 * z - 1.0) + e[1] * np.cos(2.0 * np.pi * (z + phi[0])) + e[2] * np.cos(2.0 * np.pi * (2.0 * z + phi[1]))
    out[0] = 10.0 ** (g / 10.0) if eq else 1.0
    out[1] = 10.0 ** ((-level_db + tilt * (k - (F - 1) / 2.0) / bins_per_octave) / 10.0) if noise else 0.0
    return out.astype(np.float32)


class SpecAugment(_Augment):
    """Spectrogram augmentation: per clip a smooth equaliser curve of at most eq_db dB applied as a per-bin gain that respects
    the front end's floor, a tilted noise floor noise_db = (lo, hi) dB below the clip's peak, the front end's re-normalisation to the new peak, and
    mask_count masks of up to mask_time frames and mask_freq bins each (SpecAugment), by csrc/a2s_specaug.hip.  No target changes.

    cfg: the transcription module's configuration (freq_bins); seed: the run's; device: where the batches live.  The host draws the curve, the noise
    level and tilt and sixteen 32-bit words per clip from the object's own Generator (seeded from (seed, rank, epoch) and a constant of its own), every
    quantity for every clip whether its component is on or not; content, floor, peak and the masks' places are found on the device: nothing is read
    back."""

    flags = (("eq_augment_db", 0.0), ("noise_augment_db", None), ("mask_time", 0), ("mask_freq", 0), ("mask_count", 2))
    needs = "--eq_augment_db / --noise_augment_db / --mask_time / --mask_freq need"
    cache, summary = "_specaug", "spec_augment"
    count_names, stats = ("clips", "time_masked", "freq_masked"), ("specaug_clips", "specaug_time_masked_clips", "specaug_freq_masked_clips")
    _stream = (_SPECAUG_STREAM,)

    @classmethod
    def read(cls, hparams):
        """The constructor's settings as the run's hparams state them, or None when every component is off; ValueError where one is out of range."""
        E, noise, Wt, Wf, m = check_specaug(*cls._flag_values(hparams))
        if not (E or noise is not None or Wt or Wf):
            return None
        return dict(eq_db=E, noise_db=noise, mask_time=Wt, mask_freq=Wf, mask_count=m, bins_per_octave=getattr(hparams, "bins_per_octave", 60))

    def settings(self):
        return dict(eq_db=self.E, noise_db=list(self.noise) if self.noise is not None else None, mask_time=self.Wt, mask_freq=self.Wf, mask_count=self.m)

    def __init__(self, cfg, eq_db=0.0, noise_db=None, mask_time=0, mask_freq=0, mask_count=2, seed=0, device="cpu", bins_per_octave=60, rank=0):
        self.E, self.noise, self.Wt, self.Wf, self.m = check_specaug(eq_db, noise_db, mask_time, mask_freq, mask_count)
        super().__init__(cfg, seed, device, rank)
        self.bins_per_octave = float(bins_per_octave)
        if not self.bins_per_octave >= 1:
            raise ValueError(f"spectrogram augmentation: bins_per_octave must be >= 1 (got {bins_per_octave!r})")

    @property
    def active(self):
        """Whether any component is on (the recipe builds no augmenter otherwise)."""
        return bool(self.E > 0 or self.noise is not None or self.Wt > 0 or self.Wf > 0)

    def draw_raw(self, B):
        """The next batch's draws as they leave the generator, in this fixed order: e (B, 3) in [-1, 1), phi (B, 2) in [0, 1), the noise level's
        u (B,) in [0, 1), the tilt's (B,) in [-1, 1), words (B, 16) uint32.  Nothing depends on which components are on."""
        rng = self._rng
        return (rng.uniform(-1.0, 1.0, size=(B, 3)), rng.random(size=(B, 2)), rng.random(size=B), rng.uniform(-1.0, 1.0, size=B),
                rng.integers(0, 2 ** 32, size=(B, 16), dtype=np.uint32))

    def draw(self, B):
        """(table (B, 2, F) float32, draws (B, 16) uint32) of the next batch; host only."""
        e, phi, ul, ut, words = self.draw_raw(B)
        lo, hi = self.noise if self.noise is not None else NOISE_DB_RANGE
        table = np.empty((B, 2, self.freq_bins), dtype=np.float32)
        for b in range(B):
            table[b] = specaug_table(self.freq_bins, e[b] * (self.E / 3.0), phi[b], lo + ul[b] * (hi - lo), ut[b] * NOISE_TILT_DB_PER_OCTAVE,
                                     self.bins_per_octave, eq=self.E > 0, noise=self.noise is not None)
        return table, words

    def apply(self, batch, table, draws):
        """The batch (features (B, 1, T, F) float32 on the device first) under the given table and draws: two launches on the current stream.  Returns
        the batch with a NEW feature tensor; everything else is the same objects, untouched."""
        from piano_a2s_amd import hip
        batch, x = self._features(batch)
        B = x.shape[0]
        table, draws = np.asarray(table), np.asarray(draws)
        if table.shape != (B, 2, self.freq_bins) or draws.shape != (B, 16):
            raise A2SError(f"SpecAugment: a table of shape {table.shape} and draws of shape {draws.shape} for {B} clips of {self.freq_bins} bins")
        t_dev = self._stage(table, np.float32)
        d_dev = self._stage(np.ascontiguousarray(draws, dtype=np.uint32).view(np.int32), np.int32)
        content = torch.empty(B, dtype=torch.int32, device=self.device)
        plan = torch.empty((B, 16), dtype=torch.int32, device=self.device)
        stats = torch.empty((B, 2), dtype=torch.float32, device=self.device)
        x = x.contiguous()
        hip.specaug_plan(x, t_dev, d_dev, self.Wt, self.Wf, self.m, content, plan, stats, self._count_tensor())
        batch[0] = hip.specaug_apply(x, t_dev, content, plan, stats)          # one fresh tensor per batch, as the un-augmented path's input is
        self.last_plan = (content, plan, stats)          # (device tensors; reading them synchronises -- tests and tools only)
        return batch
