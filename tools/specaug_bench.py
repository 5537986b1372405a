"""The spectrogram augmentation, measured on the MI355X: python tools/specaug_bench.py [out.json] [step_ms] [quick]

1. kernel time at B = 256, rows = 1201, F = 480, 3 warm-up + 10 timed launches between device events, median / min / max: a2s_specaug_plan on full
   windows and on windows padded behind 60 % content, a2s_specaug_apply, and, for scale and ALTERNATING with it in one process, a2s_shift_bins and
   a2s_stretch_frames on the same tensors and a plain-torch restatement of plan + apply; bytes moved (the plan reads the content twice and a chunk for
   the scan, the apply reads and writes once), TB/s and the share of the 8 TB/s roof;
2. both launches as a share of a training step: `step_ms` is the step's milliseconds from a `bench.py` run made beside this one (same batch);
3. parity: max |device - float64 oracle| on 4 clips of 201 rows with gains, noise and masks, and max |device - torch restatement| at the full size;
4. physics: for 8 rendered clips and y[n] = x[n] + c x[n - 1], c in {-0.9, -0.5, 0.5, 0.9}, the ratio of mean |augmented dry features - features of
   the filtered waveform| to mean |dry features - features of the filtered waveform|, the filter's closed-form gain table applied by the kernels.
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import specaug_oracle as oracle                                                      # noqa: E402
from tools.transpose_augment_bench import HBM_ROOF_GBS, _alternating, _stats, _timed          # noqa: E402

FILTERS = (-0.9, -0.5, 0.5, 0.9)
K8 = 8.0 * float(np.log2(10.0))


def torch_specaug(x, table, content, plan):
    """The definition in plain torch, fp32: content and the mask plan are taken from the kernel's plan (integer work), everything on the features
    is restated: floor, powers, peak, logarithm, masks."""
    B, rows, F = x.shape
    t = torch.arange(rows, device=x.device).view(1, rows, 1)
    k = torch.arange(F, device=x.device).view(1, 1, F)
    live = t < content.view(B, 1, 1)
    x_min = torch.where(live, x, torch.full_like(x, float("inf"))).amin(dim=(1, 2), keepdim=True)
    p_min = torch.exp2((x_min - 1.0) * K8)
    q = torch.where(x - x_min <= 2.0 ** -18, torch.zeros_like(x), table[:, :1] * torch.exp2((x - 1.0) * K8))
    y = torch.maximum(p_min, q + table[:, 1:])
    M = torch.where(live, y, torch.zeros_like(y)).amax(dim=(1, 2), keepdim=True)
    out = (1.0 + torch.log2(y / M) * (float(np.log10(2.0)) / 8.0)).clamp(0.0, 1.0)
    keep = live.expand(B, rows, F).clone()
    for i in range(4):
        t0, w, k0, wk = (plan[:, j].view(B, 1, 1) for j in (2 * i, 2 * i + 1, 8 + 2 * i, 9 + 2 * i))
        keep &= ~((t >= t0) & (t < t0 + w)) & ~((k >= k0) & (k < k0 + wk))
    return torch.where(keep, out, torch.zeros_like(out))


def _buffers(B, dev):
    return (torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 16), dtype=torch.int32, device=dev), torch.empty((B, 2), device=dev),
            torch.zeros(3, dtype=torch.int32, device=dev))


def _draws(B, F, rng, dev):
    tab = np.stack([oracle.table(F, rng.uniform(-2, 2, 3), rng.random(2), rng.uniform(30, 60), rng.uniform(-3, 3), 60) for _ in range(B)])
    words = rng.integers(0, 2 ** 32, size=(B, 16), dtype=np.uint32)
    return tab, words, torch.from_numpy(tab).to(dev), torch.from_numpy(words.view(np.int32).copy()).to(dev)


def kernel_times(dev, B, rows, F=480):
    from piano_a2s_amd import hip
    rng = np.random.default_rng(5)
    x = torch.rand(B, rows, F, device=dev).clamp_(min=0.33)
    y = torch.empty_like(x)
    _, _, tab, words = _draws(B, F, rng, dev)
    content, plan, stats, counters = _buffers(B, dev)
    n = x.numel() * 4
    out = {"batch": B, "rows": rows, "freq_bins": F, "feature_bytes": n}
    padded = x.clone()
    padded[:, (6 * rows) // 10:] = 0
    for name, t, read in (("full", x, 2 * n + B * min(16, rows) * F * 4), ("padded_behind_60_percent", padded, int(2 * 0.6 * n + 0.4 * n))):
        ms = _stats(_timed(lambda: hip.specaug_plan(t, tab, words, 100, 60, 2, content, plan, stats, counters)))
        out[f"specaug_plan_{name}"] = {"ms": ms, "bytes_read": read, "tb_per_s": read / (ms["median"] * 1e-3) / 1e12}
    del padded
    hip.specaug_plan(x, tab, words, 100, 60, 2, content, plan, stats, counters)
    ref = torch_specaug(x, tab, content, plan)
    hip.specaug_apply(x, tab, content, plan, stats, y=y)
    out["max_abs_diff_kernel_vs_torch_fp32"] = float((y - ref).abs().max())
    del ref
    eff = torch.from_numpy(np.where(np.arange(B) % 2 == 0, 5.0 * rng.integers(-6, 7, size=B), rng.uniform(-32.5, 32.5, size=B)).astype(np.float32)).to(dev)
    step = torch.from_numpy(np.rint(65536.0 / rng.uniform(0.85, 1.15, size=B)).astype(np.int32)).to(dev)
    fns = [lambda: hip.specaug_apply(x, tab, content, plan, stats, y=y), lambda: hip.shift_bins(x, eff, y=y), lambda: hip.stretch_frames(x, step, y=y),
           lambda: torch_specaug(x, tab, content, plan)]
    a, s, f, t = (_stats(ms) for ms in _alternating(fns))
    tbs = lambda v: 2 * n / (v["median"] * 1e-3) / 1e12
    out["specaug_apply"] = {"ms": a, "bytes_moved": 2 * n, "tb_per_s": tbs(a), "share_of_8tb_roof": tbs(a) * 1e3 / HBM_ROOF_GBS}
    out["shift_bins"] = {"ms": s, "tb_per_s": tbs(s)}
    out["stretch_frames"] = {"ms": f, "tb_per_s": tbs(f)}
    out["torch_restatement_of_plan_and_apply"] = {"ms": t}
    out["apply_over_shift_bins"] = a["median"] / s["median"]
    return out


def parity(dev, rows=201, F=480):
    from piano_a2s_amd import hip
    rng = np.random.default_rng(9)
    B = 4
    x = np.maximum(np.float32(0.33), rng.random((B, rows, F)).astype(np.float32))
    x[1, rows // 2:] = 0
    tab_h, words_h, tab, words = _draws(B, F, rng, dev)
    content, plan, stats, counters = _buffers(B, dev)
    xd = torch.from_numpy(x).to(dev)
    hip.specaug_plan(xd, tab, words, 20, 30, 2, content, plan, stats, counters)
    got = hip.specaug_apply(xd, tab, content, plan, stats).cpu().numpy().astype(np.float64)
    err = max(float(np.abs(got[b] - oracle.apply(x[b], tab_h[b], oracle.mask_plan(oracle.content_rows(x[b]), F, words_h[b], 20, 30, 2))["out"]).max())
              for b in range(B))
    return {"clips": B, "rows": rows, "max_abs_diff_kernel_vs_float64_oracle": err}


def physics(dev, clips):
    from piano_a2s_amd import hip, scoregen
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    front = VQT(dev)
    progs = np.stack([scoregen.pack_program(c, rows=scoregen.MAX_EVENTS) for c in clips])
    wave = render(torch.from_numpy(progs).to(dev))
    dry = front(wave).contiguous()
    B, F = dry.shape[0], dry.shape[-1]
    out = {}
    for c in FILTERS:
        w = wave.clone()
        w[..., 1:] += c * wave[..., :-1]
        wet = front(w)
        tab = torch.from_numpy(np.stack([oracle.filter_gain_table(c, F)] * B)).to(dev)
        content, plan, stats, counters = _buffers(B, dev)
        hip.specaug_plan(dry, tab, torch.zeros((B, 16), dtype=torch.int32, device=dev), 0, 0, 1, content, plan, stats, counters)
        aug = hip.specaug_apply(dry, tab, content, plan, stats)
        with_aug = (aug - wet).abs().flatten(1).mean(dim=1)
        without = (dry - wet).abs().flatten(1).mean(dim=1)
        ratios = (with_aug / without).cpu().tolist()
        out[str(c)] = {"ratio_per_clip": ratios, "worst": max(ratios), "mean_abs_augmented_db": float(80 * with_aug.mean()), "mean_abs_dry_db": float(80 * without.mean())}
    return {"clips": B, "frames": int(dry.shape[-2]), "per_filter": out}


def main():
    from piano_a2s_amd import scoregen, spec
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "specaug.json")
    step_ms = float(sys.argv[2]) if len(sys.argv) > 2 and float(sys.argv[2]) > 0 else None
    quick = len(sys.argv) > 3 and sys.argv[3] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("specaug_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n_clips, B, rows = (2, 8, 201) if quick else (8, 256, 1201)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["kernels"] = kernel_times(dev, B, rows)
    if step_ms:
        k = res["kernels"]
        both = k["specaug_plan_full"]["ms"]["median"] + k["specaug_apply"]["ms"]["median"]
        res["training_step"] = {"step_ms": step_ms, "augmentation_ms": both, "share_of_step": both / step_ms}
    res["parity"] = parity(dev)
    res["physics"] = physics(dev, [scoregen.make_clip(spec.default_cfg(max_bars=2), seed, frames=301) for seed in (3, 7, 11, 13, 17, 19, 23, 29)][:n_clips])
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
