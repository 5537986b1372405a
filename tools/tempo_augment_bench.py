"""The tempo augmentation, measured on the MI355X: python tools/tempo_augment_bench.py [out.json] [step_ms] [quick]

1. kernel time at B = 256, rows = 1201, F = 480, 3 warm-up + 10 timed launches between device events, median / min / max:
   a2s_tempo_plan on windows that are full and on windows padded behind 60 % content;
   a2s_stretch_frames with per-clip factors uniform in 1 +- 0.15 and in 1 +- 0.25, and, for scale and ALTERNATING with it in one process, a2s_shift_bins
   on the same tensors (the kernel of section 16: the same bytes, no reuse between rows) and a plain-torch composition (per-clip gather of two rows
   + lerp); algorithmic GB/s (one read and one write of the features) and the share of the 8 TB/s roof;
2. both launches as a share of a training step: `step_ms` is the step's milliseconds from a `bench.py` run made beside this one (same batch);
3. how good "a tempo change is a resampling of the frames" is: 32 full-length rendered clips without their noise floor, for c in 0.8 .. 1.2 the
   features of the clip rendered with every onset and length scaled by c against the stretched features of the clip as drawn (and against the
   unstretched ones, as a control): mean and 95th percentile in dB (x 80), and the ratio of the means.
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.transpose_augment_bench import HBM_ROOF_GBS, _alternating, _stats, _timed          # noqa: E402

FACTORS = (0.80, 0.90, 0.95, 1.05, 1.10, 1.20)


def torch_stretch(x, step):
    """Linear interpolation along time in plain torch: per clip a gather of the two neighbouring rows and a lerp (what the kernel does for
    step <= 65536; for larger steps the kernel's third tap has no counterpart here, so this moves no more bytes than the kernel does)."""
    B, rows, F = x.shape
    pos = torch.arange(rows, device=x.device, dtype=torch.int64).view(1, rows) * step.long().view(B, 1)
    k0, a = pos >> 16, ((pos & 65535).float() / 65536.0).view(B, rows, 1)
    taps = []
    for k in (k0, k0 + 1):
        ok = (k < rows).view(B, rows, 1)
        taps.append(torch.gather(x, 1, k.clamp(max=rows - 1).view(B, rows, 1).expand_as(x)) * ok)
    return torch.lerp(taps[0], taps[1], a)


def kernel_times(dev, B, rows, F=480):
    from piano_a2s_amd import hip
    rng = np.random.default_rng(5)
    x = torch.rand(B, rows, F, device=dev)
    y = torch.empty_like(x)
    nbytes = 2 * x.numel() * 4
    out = {"batch": B, "rows": rows, "freq_bins": F, "bytes_per_call": nbytes}
    # the plan: full windows cost one chunk per clip, padded windows their padding
    u = torch.from_numpy(rng.random(size=B, dtype=np.float32)).to(dev)
    content, step = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    counters = torch.zeros(3, dtype=torch.int32, device=dev)
    padded = x.clone()
    padded[:, (6 * rows) // 10:] = 0
    for name, t in (("full", x), ("padded_behind_60_percent", padded)):
        ms = _timed(lambda: hip.tempo_plan(t, u, 0.15, min(400, rows // 3), content, step, counters))
        out[f"tempo_plan_{name}_ms"] = _stats(ms)
        out[f"tempo_plan_{name}_content"] = sorted(set(content.tolist()))
        out[f"tempo_plan_{name}_step_range"] = [int(step.min()), int(step.max())]
    del padded
    eff = torch.from_numpy(np.where(np.arange(B) % 2 == 0, 5.0 * rng.integers(-6, 7, size=B), rng.uniform(-32.5, 32.5, size=B)).astype(np.float32)).to(dev)
    for R in (0.15, 0.25):
        c = rng.uniform(1.0 - R, 1.0 + R, size=B)
        st = torch.from_numpy(np.rint(65536.0 / c).astype(np.int32)).to(dev)
        ref = torch_stretch(x, st)
        hip.stretch_frames(x, st, y=y)
        expand = (st <= 65536).view(B, 1, 1)
        err = float(((y - ref) * expand).abs().max())          # (the two agree where both interpolate linearly)
        del ref
        k_ms, s_ms, t_ms = _alternating([lambda: hip.stretch_frames(x, st, y=y), lambda: hip.shift_bins(x, eff, y=y), lambda: torch_stretch(x, st)])
        k, s, t = _stats(k_ms), _stats(s_ms), _stats(t_ms)
        gbs = lambda v: nbytes / (v["median"] * 1e-3) / 1e9
        out[f"R_{R}"] = {"step_range": [int(st.min()), int(st.max())], "max_abs_diff_kernel_vs_torch_where_step_le_65536": err,
                         "stretch_frames_ms": k, "shift_bins_ms": s, "torch_gather_lerp_ms": t,
                         "stretch_frames_gb_per_s": gbs(k), "shift_bins_gb_per_s": gbs(s), "torch_gb_per_s": gbs(t),
                         "stretch_frames_share_of_8tb_roof": gbs(k) / HBM_ROOF_GBS, "stretch_over_shift": k["median"] / s["median"],
                         "larger_spread_ms": max(k["max"] - k["min"], s["max"] - s["min"])}
    return out


def scaled_program(clip, c, rows):
    """The clip's render program without its noise floor, every event's onset and length multiplied by c (rounded to samples)."""
    from piano_a2s_amd import scoregen
    p = scoregen.pack_program(clip, rows=rows).copy()
    p[0, 6] = np.array(0.0, dtype=np.float32).view(np.int32)
    n = len(clip["events"])
    p[1:1 + n, 0] = np.rint(p[1:1 + n, 0] * c).astype(np.int32)
    p[1:1 + n, 1] = np.rint(p[1:1 + n, 1] * c).astype(np.int32)
    return p


def fidelity(dev, clips):
    from piano_a2s_amd import hip, scoregen
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    front = VQT(dev)
    rows = scoregen.MAX_EVENTS
    feats = {c: front(render(torch.from_numpy(np.stack([scaled_program(clip, c, rows) for clip in clips])).to(dev))) for c in (1.0,) + FACTORS}
    drawn = feats[1.0].contiguous()
    B = drawn.shape[0]
    out = {}
    for c in FACTORS:
        stretched = hip.stretch_frames(drawn, torch.full((B,), int(np.rint(65536 / c)), dtype=torch.int32, device=dev))
        row = {"step": int(np.rint(65536 / c)),
               "clips_whose_content_leaves_the_window": int(sum((cl["events"][:, 0] + cl["events"][:, 1]).max() * c > cl["n_samples"] for cl in clips))}
        for name, t in (("stretched", stretched), ("unstretched", drawn)):
            e = (80.0 * (t - feats[c]).abs()).flatten().cpu().numpy()
            row[name + "_mean_db"], row[name + "_p95_db"] = float(e.mean()), float(np.percentile(e, 95))
        row["ratio_of_means"] = row["stretched_mean_db"] / row["unstretched_mean_db"]
        out[str(c)] = row
    return {"clips": B, "frames": int(drawn.shape[2]), "per_factor": out}


def main():
    from piano_a2s_amd import scoregen, spec
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tempo_augment.json")
    step_ms = float(sys.argv[2]) if len(sys.argv) > 2 and float(sys.argv[2]) > 0 else None
    quick = len(sys.argv) > 3 and sys.argv[3] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("tempo_augment_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cfg = spec.default_cfg()
    n_clips, B, rows = (2, 8, 201) if quick else (32, 256, 1201)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["kernels"] = kernel_times(dev, B, rows)
    if step_ms:
        k = res["kernels"]
        both = k["R_0.15"]["stretch_frames_ms"]["median"] + k["tempo_plan_full_ms"]["median"]
        res["training_step"] = {"step_ms": step_ms, "augmentation_ms": both, "share_of_step": both / step_ms,
                                "with_padded_windows_ms": k["R_0.15"]["stretch_frames_ms"]["median"] + k["tempo_plan_padded_behind_60_percent_ms"]["median"]}
    res["fidelity_db"] = fidelity(dev, [scoregen.make_clip(cfg, 1234 + i, frames=rows) for i in range(n_clips)])
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
