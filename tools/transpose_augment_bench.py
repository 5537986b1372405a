"""The transposition augmentation, measured on the MI355X: python tools/transpose_augment_bench.py [out.json] [step_ms] [quick]

1. kernel time at B = 256, rows = 1201, F = 480 with per-clip shifts mixed whole and fractional: 3 warm-up + 10 timed launches between device events,
   median / min / max, for a2s_transpose_targets, a2s_shift_bins and a plain-torch composition of the same shift (per-clip gather + lerp), the two
   shifts ALTERNATING in one process; algorithmic GB/s (one read and one write of the features) and the share of the 8 TB/s roof;
2. both launches as a share of a training step: `step_ms` is the step's milliseconds from a `bench.py` run made beside this one (same batch);
3. how good "a transposition is a row shift" is: 32 full-length rendered clips, for every s in -6 .. 6 the features of the clip rendered s semitones
   higher against the shifted features of the clip as drawn (and against the unshifted ones, as a control): mean and 95th percentile in dB (x 80);
4. the share of clips left un-transposed: one epoch of the rendered corpus, and the on-disk fixture corpus of tests/disk_corpus.py.
`quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_GBS = 8000.0


def _timed(fn, warmup=3, reps=10, before=None):
    """Milliseconds of each of `reps` calls, every call between two device events of its own, after `warmup` calls; `before` runs ahead of every
    call, in front of the first event."""
    out = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return out


def _alternating(fns, warmup=3, reps=10):
    """As _timed for several functions, taking turns call by call: what disturbs one disturbs the others."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(reps):
        for fn, o in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            o.append(a.elapsed_time(b))
    return out


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "calls": [float(v) for v in ms]}


def torch_shift(x, eff):
    """The same operation in plain torch: per clip a gather of the two taps and a lerp."""
    B, F = x.shape[0], x.shape[-1]
    m = torch.floor(eff)
    a = (eff - m).view(B, 1, 1)
    j = torch.arange(F, device=x.device).view(1, 1, F) - m.long().view(B, 1, 1)
    taps = []
    for src in (j, j - 1):
        ok = (src >= 0) & (src < F)
        taps.append(torch.gather(x, 2, src.clamp(0, F - 1).expand_as(x)) * ok)
    return torch.lerp(taps[0], taps[1], a)


def clip_targets(clips, cfg):
    from piano_a2s_amd.synthetic import pad_measure
    U, L = cfg["max_length"]
    key = torch.tensor([c.get("keys") or [c["key"]] * cfg["max_bars"] for c in clips], dtype=torch.long)
    upper = torch.from_numpy(np.stack([np.stack([pad_measure(ids, U) for ids in c["ids"]["upper"]]) for c in clips]))
    lower = torch.from_numpy(np.stack([np.stack([pad_measure(ids, L) for ids in c["ids"]["lower"]]) for c in clips]))
    return key, upper, lower


def kernel_times(dev, B, rows, clips, cfg):
    from piano_a2s_amd import hip, kern_transpose
    F = 480
    rng = np.random.default_rng(5)
    n = np.where(np.arange(B) % 2 == 0, 5.0 * rng.integers(-6, 7, size=B), rng.uniform(-32.5, 32.5, size=B)).astype(np.float32)
    eff = torch.from_numpy(n).to(dev)
    x = torch.rand(B, rows, F, device=dev)
    y = torch.empty_like(x)
    ref = torch_shift(x, eff)
    hip.shift_bins(x, eff, y=y)
    err = float((y - ref).abs().max())
    del ref
    k_ms, t_ms = _alternating([lambda: hip.shift_bins(x, eff, y=y), lambda: torch_shift(x, eff)])
    nbytes = 2 * x.numel() * 4
    k, t = _stats(k_ms), _stats(t_ms)
    spread = max(k["max"] - k["min"], t["max"] - t["min"])
    tables = [torch.from_numpy(np.array(tab)).to(dev) for tab in kern_transpose.tables()]
    key, upper, lower = (v.to(dev) for v in clip_targets([clips[i % len(clips)] for i in range(B)], cfg))
    s = torch.from_numpy(rng.integers(-6, 7, size=B).astype(np.int32)).to(dev)
    d = torch.from_numpy(rng.uniform(-2.5, 2.5, size=B).astype(np.float32)).to(dev)
    e2, counters = torch.empty(B, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    keep = (key.clone(), upper.clone(), lower.clone())

    def restore():                        # the kernel rewrites in place: every timed call starts from the clips as drawn (copies in front of the first event)
        for dst, src in zip((key, upper, lower), keep):
            dst.copy_(src)

    tt = _stats(_timed(lambda: hip.transpose_targets(*tables, s, d, key, upper, lower, 5, e2, counters), before=restore))
    return {"batch": B, "rows": rows, "freq_bins": F, "bytes_per_call": nbytes, "max_abs_diff_kernel_vs_torch": err,
            "shift_bins_ms": k, "torch_gather_lerp_ms": t, "larger_spread_ms": spread,
            "kernel_faster_by_more_than_the_spread": bool(t["median"] - k["median"] > spread),
            "shift_bins_gb_per_s": nbytes / (k["median"] * 1e-3) / 1e9, "torch_gb_per_s": nbytes / (t["median"] * 1e-3) / 1e9,
            "shift_bins_share_of_8tb_roof": nbytes / (k["median"] * 1e-3) / 1e9 / HBM_ROOF_GBS,
            "transpose_targets_ms": tt, "target_tokens_per_clip": int(upper[0].numel() + lower[0].numel())}


def transposed_program(clip, s, rows):
    """The clip's render program with every event s semitones higher: only the phase increments change (instrument, amplitudes, decays as drawn)."""
    from piano_a2s_amd import scoregen
    p = scoregen.pack_program(clip, rows=rows).copy()
    for i, (_, _, midi) in enumerate(clip["events"], 1):
        p[i, 2] = np.array(scoregen.inc1(int(midi) + s), dtype=np.uint32).view(np.int32)
    return p


def approximation(dev, clips):
    from piano_a2s_amd import hip, scoregen
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    front = VQT(dev)
    rows = scoregen.MAX_EVENTS
    feats = {s: front(render(torch.from_numpy(np.stack([transposed_program(c, s, rows) for c in clips])).to(dev))) for s in range(-6, 7)}
    drawn = feats[0].contiguous()
    B, F = drawn.shape[0], drawn.shape[-1]
    out = {}
    for s in range(-6, 7):
        shifted = hip.shift_bins(drawn, torch.full((B,), 5.0 * s, device=dev))
        lo, hi = (5 * s, F) if s >= 0 else (0, F + 5 * s)
        row = {}
        for name, t in (("shifted", shifted), ("unshifted", drawn)):
            e = (80.0 * (t - feats[s])[..., lo:hi].abs()).flatten().cpu().numpy()
            row[name + "_mean_db"], row[name + "_p95_db"] = float(e.mean()), float(np.percentile(e, 95))
        out[str(s)] = row
    return {"clips": B, "frames": int(drawn.shape[2]), "per_semitone": out}


def unrepresentable(dev, clips, cfg, K_values):
    """One pass over `clips` per K with the augmenter's own draws (epoch 0, rank 0): the device's counters."""
    from piano_a2s_amd import hip, kern_transpose
    from piano_a2s_amd.augment import TransposeAugment
    tables = [torch.from_numpy(np.array(tab)).to(dev) for tab in kern_transpose.tables()]
    key, upper, lower = clip_targets(clips, cfg)
    out = {}
    for K in K_values:
        aug = TransposeAugment(cfg, K, 0.0, seed=1234, device=dev)
        aug.reseed(0, 0)
        s, d = aug.draw(len(clips))
        counters = torch.zeros(3, dtype=torch.int32, device=dev)
        hip.transpose_targets(*tables, torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), key.to(dev), upper.to(dev), lower.to(dev), 5,
                              torch.empty(len(clips), device=dev), counters)
        c = counters.tolist()
        out[str(K)] = {"clips": c[0], "transposed": c[1], "not_representable": c[2], "drawn_s_nonzero": int((s != 0).sum())}
    return out


def fixture_corpus_clips(cfg, n):
    """The scores of the on-disk fixture corpus tests/disk_corpus.py writes (ASAP layout), as clips of the shape the generator returns."""
    from tests import disk_corpus
    with tempfile.TemporaryDirectory() as root:
        written = disk_corpus.write_asap_corpus(root, cfg, "train", n, 41, 1234)
    return [{"keys": [int(bar[0]) + 6 for bar in score], "ids": {"upper": [bar[3] for bar in score], "lower": [bar[2] for bar in score]}} for _, score in written.values()]


def main():
    from piano_a2s_amd import scoregen, spec
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "transpose_augment.json")
    step_ms = float(sys.argv[2]) if len(sys.argv) > 2 and float(sys.argv[2]) > 0 else None
    quick = len(sys.argv) > 3 and sys.argv[3] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("transpose_augment_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cfg = spec.default_cfg()
    n_epoch, n_approx, B, rows = (64, 2, 8, 201) if quick else (1024, 32, 256, 1201)
    clips = [scoregen.make_clip(cfg, 1234 + i, frames=rows) for i in range(n_epoch)]
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["kernels"] = kernel_times(dev, B, rows, clips, cfg)
    if step_ms:
        both = res["kernels"]["shift_bins_ms"]["median"] + res["kernels"]["transpose_targets_ms"]["median"]
        res["training_step"] = {"step_ms": step_ms, "augmentation_ms": both, "share_of_step": both / step_ms}
    res["approximation_db"] = approximation(dev, clips[:n_approx])
    fixture = fixture_corpus_clips(spec.default_cfg(freq_bins=24, conv_feature_size=32, hidden_size=32, max_length=(12, 8)), 16 if quick else 64)
    res["unrepresentable"] = {"rendered_corpus": unrepresentable(dev, clips, cfg, (1, 2, 3, 6)),
                              "disk_fixture_corpus": unrepresentable(dev, fixture, spec.default_cfg(max_length=(12, 8)), (1, 2, 3, 6))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
