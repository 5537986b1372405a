"""ONE ConvStack call -- Engine.convstack(S, x, training, drop_mask), then engine_bwd._convstack_bwd, exactly as Engine.forward and engine_bwd.backward
issue them -- against the float64 oracle of tests/convstack_oracle.py, on every path the call can take: each forced by its switch and proved by the
plan (conv_bwd_plan.plan_convstack_bwd recomputed from the library's own eligibility answers), by the launch helpers of piano_a2s_amd/hip.py the
executor went through (wrapped for the duration of the call: names and deciding arguments) and by the library's launch counters.

Compared per tensor.  Forward: the four pre-BatchNorm outputs, the 5 x 4 BatchNorm vectors, z, out, the operand ranges (yabs exact, abound to 2^-22
and not below the activations), the updated running statistics (num_batches_tracked exact).  Backward: the 15 parameter gradients.

ReLU flips.  The gradients are discontinuous where a pre-activation crosses the ReLU threshold, and no input of the sizes needed here keeps every
float64 pre-activation away from it (tests/test_convstack_oracle_cpu.py counts them).  The backward comparison therefore takes the DEVICE's
decisions: oracle.masks_from_saved recomputes them from the device's saved fp32 tensors, and oracle.gradients(masks=...) differentiates under them.
That is sound only where a device decision that differs from the float64 oracle's lies within FLIP_MARGIN standard deviations of the threshold in
the oracle; every other difference fails the test and names the element.  The flips per layer are reported.

How the kernels form the decision.  Every kernel that masks a gradient or stages an activation evaluates x * scale + shift as ONE fma: the
row-streaming, Linear and GEMM staging kernels write fmaf(...) (csrc/a2s_conv_rows.hip, a2s_conv_wrows.hip, a2s_linear.hip, a2s_gemm.hip); the tiled
convolutions (csrc/a2s_conv.hip, a2s_conv_wgrad.hip), the BatchNorm backward kernels (a2s_bn.hip) and the GEMM statistics epilogue (a2s_gemm.hip) write the plain expression, which
hipcc contracts (its default for device code is -ffp-contract=fast-honor-pragmas and piano_a2s_amd/build.py passes no other; a probe kernel with that
expression compiles to a single v_fma_f32 for gfx950).  So double(y) * double(scale) + double(shift) > 0 is the decision of every kernel and no
element is ambiguous; the number of elements at which a two-rounding evaluation would have decided otherwise is reported beside the flips.

Bars: per tensor, max(project bar, 3 x the deviation of the oracle's own float32 evaluation from its float64 one) -- the rule of
test_gpu_encoder_call.py; project bars, all as max |got - ref| / max |ref|: 5e-6 forward tensors and BatchNorm vectors (test_gpu_ops.py),
1e-5 running statistics (same file), 2e-5 gradients (test_gpu_bwd_ops.py).  Every figure goes, with the float32 deviation and the bar used, to the
file test_gpu_ops.py::_report writes, under labels beginning "convstack_call".

The inputs' preconditions (flip margins, share near the threshold, the float32 oracle's own flips, BatchNorm variances) are asserted on the CPU by
tests/test_convstack_oracle_cpu.py over CASES / INPUTS below.  rows = B * T = 1 in training mode is undefined in torch (the unbiased variance of one
value) and is left out."""
import contextlib
import functools
import inspect
import os

import pytest
import torch

from tests import convstack_oracle as oracle
from tests.test_gpu_operand_ranges import CHAIN_GAMMAS, CHAIN_MARGIN

pytestmark = pytest.mark.gpu

CF = 256                                     # conv_feature_size: the Linear's kernels need N = 256
FWD_BAR, STAT_BAR, GRAD_BAR = 5e-6, 1e-5, 2e-5
WEIGHTS_SEED = 23
NEAR_SHARE = 1e-4                            # precondition (b): at most this share of a layer's float64 pre-activations within FLIP_MARGIN of the threshold

# (B, T, F): the smallest shapes at which each mechanism can still go wrong
CASES = [
    (2, 64, 128),        # 128 rows: exactly one 128-row block of the own Linear data gradient -> "own", layer 4 on "rows" with the scalar range; four 16-row strips; F tiles 120 + 8
    (3, 43, 128),        # 129 rows; two strips of 22 and 21
    (33, 4, 160),        # 132 rows from 4-frame clips: every row next to a clip edge; F tiles 120 + 40
    (1, 127, 128),       # one clip; 127 rows, one short of the own kernel: "generic"; seven strips of 20, the last of 7 rows
    (5, 13, 128),        # 65 rows: the first row count with the statistics epilogue
    (4, 16, 128),        # 64 rows: "gemm", no partials, layer 4 on statistics of its own and "apply"; the smallest M of the own Linear weight gradient
    (3, 21, 128),        # 63 rows: the Linear weight gradient falls back to _linear_bwd
    (3, 23, 132),        # F % 4 == 0, F % 32 != 0: row kernels, all three Linear kernels ineligible
    (3, 9, 130),         # F % 4 != 0: no row kernel, generic conv1, tiled everything, "gemm"
    (3, 23, 24),         # F < 128
    (2, 1, 128),         # T = 1: only the middle kernel row contributes
    (1, 2, 128),         # one clip of two frames
    (2, 129, 128),       # 258 rows: three Linear blocks, the last of two rows; more than four 64-row weight-gradient blocks
    # added to the issue's list: the model's own F.  conv1's compile-time-shaped weight gradient (conv3x3_wgrad_c1_stream<20, 480>, csrc/a2s_conv_wgrad.hip) is
    # launched at F == 480 only, so no case above reaches it; F tiles 4 x 120
    (2, 3, 480),
]
PATH_CASES = [(3, 43, 128), (1, 127, 128), (3, 23, 132)]
BIG = (2, 64, 128)
SMALL = (3, 23, 132)                         # the eval and dropout calls
# every (case, variant) a GPU test runs: the CPU test asserts the preconditions over exactly these
INPUTS = [(c, "plain") for c in CASES] + [(BIG, "gammas"), (BIG, "small"), (SMALL, "dropout")]

# What each case is for, on the default path: the Linear's data gradient, the forms of layers 4, 3, 2, 1, their statistics sources, whether the
# Linear's own weight-gradient kernel runs and which forward kernel ("f64": at most 64 rows in training mode, Engine.convstack).  From reading conv_bwd_plan.py and the *_ok predicates of csrc/a2s_linear.hip; the test
# recomputes the plan from the library's answers and asserts it is this.
_ROWS = dict(forms=("rows", "rows", "rows", "tiled"), stats=("partial",) * 4)
_GENERIC = dict(dgrad="generic", forms=("apply", "rows", "rows", "tiled"), stats=("partial",) * 4)
_GEMM = dict(dgrad="gemm", forms=("apply", "rows", "rows", "tiled"), stats=("own", "partial", "partial", "partial"))
FACTS = {
    (2, 64, 128): dict(dgrad="own", **_ROWS, lin_wgrad=True, lin_fwd="own"),
    (3, 43, 128): dict(dgrad="own", **_ROWS, lin_wgrad=True, lin_fwd="own"),
    (33, 4, 160): dict(dgrad="own", **_ROWS, lin_wgrad=True, lin_fwd="own"),
    (1, 127, 128): dict(**_GENERIC, lin_wgrad=True, lin_fwd="own"),
    (5, 13, 128): dict(**_GENERIC, lin_wgrad=True, lin_fwd="own"),
    (4, 16, 128): dict(**_GEMM, lin_wgrad=True, lin_fwd="f64"),
    (3, 21, 128): dict(**_GEMM, lin_wgrad=False, lin_fwd="f64"),
    (3, 23, 132): dict(**_GENERIC, lin_wgrad=False, lin_fwd="generic"),
    # F % 4 != 0: a2s_conv3x3_wgrad_bn_ranged is not eligible, so no layer is on "rows"
    (3, 9, 130): dict(dgrad="gemm", forms=("apply", "apply", "apply", "tiled"), stats=("own", "partial", "partial", "partial"), lin_wgrad=False, lin_fwd="f64"),
    (3, 23, 24): dict(**_GEMM, lin_wgrad=False, lin_fwd="generic"),          # (period 24 is no multiple of 32, K = 960 none of 128)
    (2, 1, 128): dict(**_GEMM, lin_wgrad=False, lin_fwd="f64"),
    (1, 2, 128): dict(**_GEMM, lin_wgrad=False, lin_fwd="f64"),
    (2, 129, 128): dict(dgrad="own", **_ROWS, lin_wgrad=True, lin_fwd="own"),
    (2, 3, 480): dict(**_GEMM, lin_wgrad=False, lin_fwd="f64"),
}

# every path but the default.  Plain keys are a2s_debug_set switches; "hip.<attr>" / "bwd.<attr>" module attributes of piano_a2s_amd.hip / engine_bwd;
# "sync_bn": Engine(cfg, sync_bn=True) on a one-rank process group
PATHS = {
    "default": {},
    "conv_rows0": {"conv_rows": 0},
    "conv_rows1": {"conv_rows": 1},
    "conv_rows3": {"conv_rows": 3},
    "conv_rows0_bf16x3_0": {"conv_rows": 0, "conv_bf16x3": 0},
    "conv_rows0_f16x2_0": {"conv_rows": 0, "conv_f16x2": 0},
    "conv_rows_stage0": {"conv_rows_stage": 0},
    "conv_rows_stage1": {"conv_rows_stage": 1},
    "conv_c1_fast0": {"conv_c1_fast": 0},
    "wgrad_rows0": {"wgrad_rows": 0},
    "wgrad_rows0_f16x2_0": {"wgrad_rows": 0, "wgrad_f16x2": 0},
    "wgrad_rows0_bf16x3_0": {"wgrad_rows": 0, "wgrad_bf16x3": 0},
    "gemm_bf16x3_0": {"gemm_bf16x3": 0},
    "gemm_f16x2_0": {"gemm_f16x2": 0},
    "linear_kernels_off": {"hip.LINEAR_KERNELS": False},
    "fuse_bn_rows_off": {"bwd._FUSE_BN_ROWS": False},
    "dgrad_bnstats_off": {"bwd._DGRAD_BNSTATS": False},
    "fuse_bn_apply": {"bwd._FUSE_BN_APPLY": True},
    "fuse_bn_apply_l1_off": {"bwd._FUSE_BN_APPLY_L1": False},
    "lin_wgrad_beside": {"bwd._LIN_WGRAD_AT": "beside"},
    "lin_wgrad_at4": {"bwd._LIN_WGRAD_AT": 4},
    "lin_wgrad_at3": {"bwd._LIN_WGRAD_AT": 3},
    "lin_wgrad_at2": {"bwd._LIN_WGRAD_AT": 2},
    "sync_bn_fused": {"sync_bn": True},
    "sync_bn_unfused": {"sync_bn": True, "bwd._SYNC_FUSED": False},
}
# Paths proved by a2s_launch_count() over the call: it must differ from that of the path named here at the same case (the tiled convolutions add
# range and statistics passes to the row kernels' launches; their fp32-input and three-term forms drop the range passes again).  Measured on the
# MI355X at (3, 43, 128): default 50, conv_rows0 69, conv_rows0_bf16x3_0 and conv_rows0_f16x2_0 60.
# What is left without such a proof replaces one kernel by another in the same number of launches and has no counter: conv_rows3 (one accumulator
# set in place of two), conv_rows_stage1 (bit 1 only picks the 40 -> 40 data gradient's form), conv_c1_fast0, wgrad_rows0 with wgrad_f16x2 / wgrad_bf16x3
# off (wgrad_rows0 itself shows in the plan: the library answers that no layer is eligible for "rows"), gemm_bf16x3_0, gemm_f16x2_0.  For these the
# proof is the switch's value read back inside the path (_path) -- and that the call still holds every bar.
COUNT_DIFFERS = {"conv_rows0": "default", "conv_rows0_bf16x3_0": "conv_rows0", "conv_rows0_f16x2_0": "conv_rows0"}
COUNTERS = ("conv_rows16_c20_launches", "conv_rows_stage_launches")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def cfg(F):
    from piano_a2s_amd import spec
    return spec.default_cfg(freq_bins=F, hidden_size=16)          # (only the convstack.* entries are used, as in test_gpu_operand_ranges.chain_state)


def input_seed(B, T, F):
    return 100000 * B + 1000 * T + F


@functools.lru_cache(maxsize=None)
def inputs(B, T, F, variant="plain"):
    """Everything one call reads, on the CPU: the 15 parameters and 15 buffers of spec.procedural_state(cfg, 23), seeded randn x (B, 1, T, F) and d_out
    (B, T, 256), no dropout mask.  Variants: "gammas" -- the BatchNorm2d gammas of CHAIN_GAMMAS with their 2^+-3 per-channel spread, biases 0.3 x the
    same magnitudes (the recipe of test_gpu_operand_ranges.chain_state: every layer's range at another magnitude); "small" -- x at 1e-3 and d_out at
    1e-6 of their usual size; "dropout" -- a seeded uint8 mask that drops about a fifth of `out`."""
    from piano_a2s_amd import spec
    st = spec.procedural_state(cfg(F), WEIGHTS_SEED)
    W, buffers = oracle.convstack_tensors(st)
    W, buffers = {k: v.clone() for k, v in W.items()}, {k: v.clone() for k, v in buffers.items()}
    g = torch.Generator().manual_seed(input_seed(B, T, F))
    x, d_out, drop = torch.randn(B, 1, T, F, generator=g), torch.randn(B, T, CF, generator=g), None
    if variant == "gammas":
        for i, mag in enumerate(CHAIN_GAMMAS, start=1):
            n = W[f"convstack.bn{i}.weight"].numel()
            per = mag * torch.exp2(torch.randint(-3, 4, (n,), generator=g).float())
            W[f"convstack.bn{i}.weight"] = per * (1.0 + 0.25 * (2 * torch.rand(n, generator=g) - 1))
            W[f"convstack.bn{i}.bias"] = 0.3 * per * torch.randn(n, generator=g)
    elif variant == "small":
        x, d_out = x * 1e-3, d_out * 1e-6
    elif variant == "dropout":
        drop = (torch.rand(B * T, CF, generator=g) >= 0.2).to(torch.uint8)
    else:
        assert variant == "plain"
    return dict(W=W, buffers=buffers, x=x, d_out=d_out, drop=drop)


@functools.lru_cache(maxsize=None)
def reference(B, T, F, variant="plain", training=True):
    """(f64 forward, f64 gradients with the oracle's own decisions, f32 forward, dev32) of oracle.reference: computed once per case, shared by every
    path, left unchanged.  (The gradients under the device's decisions are recomputed per call.)"""
    i = inputs(B, T, F, variant)
    return oracle.reference(i["W"], i["buffers"], i["x"], i["drop"], training, i["d_out"] if training else None)


def flip_margins(dev32):
    """Per layer 1..5: max(CHAIN_MARGIN, 3 x the deviation of the float32 oracle's normalised pre-activation), in standard deviations of the channel.
    CHAIN_MARGIN = 7e-6 stands over the 4e-6 measured on the device (comment at test_gpu_operand_ranges.CHAIN_INPUT_SEED)."""
    return [max(CHAIN_MARGIN, 3 * dev32[f"pre{i}"]) for i in (1, 2, 3, 4, 5)]


def flips(f64, masks, margins):
    """Per layer: (number of decisions in `masks` that differ from the float64 oracle's, description of the first one that lies beyond the layer's
    margin in the oracle or None)."""
    out = []
    for i, (m, margin) in enumerate(zip(masks, margins), start=1):
        diff = m.view_as(f64[f"dec{i}"]) != f64[f"dec{i}"]
        far = diff & (f64[f"pre{i}"].abs() > margin)
        msg = None
        if bool(far.any()):
            at = oracle.unravel(int(far.flatten().nonzero()[0]), far.shape)
            msg = (f"layer {i}: the decision at {oracle.where(f'pre{i}', at)} differs from the float64 oracle's, whose pre-activation lies "
                   f"{float(f64[f'pre{i}'][at]):.3e} standard deviations from the threshold (margin {margin:.3e}); {int(far.sum())} such elements")
        out.append((int(diff.sum()), msg))
    return out


# ------------------------------------------------------------------------------------------- paths, counters, recorded calls
class _path:
    """The switches of one path set, everything put back on the way out."""
    def __init__(self, name):
        self.kv = dict(PATHS[name])

    def __enter__(self):
        from piano_a2s_amd import engine_bwd, hip
        self.L = hip.lib()
        self.mods = {"hip": hip, "bwd": engine_bwd}
        self.prev_lib, self.prev_attr = {}, {}
        try:
            for k, v in self.kv.items():
                if k == "sync_bn":
                    continue
                if "." in k:
                    mod, attr = k.split(".")
                    self.prev_attr[k] = getattr(self.mods[mod], attr)
                    setattr(self.mods[mod], attr, v)
                else:
                    self.prev_lib[k] = self.L.a2s_debug_get(k.encode())
                    hip.check(self.L.a2s_debug_set(k.encode(), v), "debug_set")
                    assert self.L.a2s_debug_get(k.encode()) == v, f"switch {k}: set to {v}, reads back {self.L.a2s_debug_get(k.encode())}"
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *a):
        for k, v in self.prev_attr.items():
            mod, attr = k.split(".")
            setattr(self.mods[mod], attr, v)
        for k, v in self.prev_lib.items():
            self.L.a2s_debug_set(k.encode(), v)


@contextlib.contextmanager
def _one_rank_group(enabled):
    """A one-rank process group, set up and torn down as test_gpu_train_step.py::test_sync_bn_single_rank_equals_local_bn does; dist.all_reduce wrapped
    so that the calls are counted (yields the list they are appended to)."""
    calls = []
    if not enabled:
        yield calls
        return
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group(backend="nccl", rank=0, world_size=1)
    real = dist.all_reduce

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    dist.all_reduce = counted
    try:
        yield calls
    finally:
        dist.all_reduce = real
        dist.destroy_process_group()


RECORDED = ("linear_forward", "linear_forward_f64", "linear", "gemm", "bn_bwd", "bn_bwd_sync", "linear_wgrad", "linear_dgrad_bnstats", "conv3x3_wgrad_bn", "conv3x3_wgrad",
            "conv3x3_dgrad")


class _record:
    """Wraps the launch helpers of piano_a2s_amd.hip (engine.py and engine_bwd.py reach them through the module) and records (name, arguments by
    name, return value) of every call, in order."""
    def __enter__(self):
        from piano_a2s_amd import hip
        self.hip, self.orig, self.calls = hip, {}, []
        for name in RECORDED:
            fn = getattr(hip, name)
            self.orig[name] = fn
            setattr(hip, name, self._wrap(name, fn))
        return self

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapped(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            rec = [name, dict(bound.arguments), None]
            self.calls.append(rec)
            rec[2] = fn(*a, **kw)
            return rec[2]
        return wrapped

    def __exit__(self, *a):
        for name, fn in self.orig.items():
            setattr(self.hip, name, fn)

    def mark(self):
        return len(self.calls)


def _plan(L, path, B, T, F, sync_bn):
    """plan_convstack_bwd recomputed from the switches in force and the library's own eligibility answers (called inside the path)."""
    from piano_a2s_amd import engine_bwd as eb, hip
    from piano_a2s_amd.conv_bwd_plan import CHANS, ConvBwdFlags, plan_convstack_bwd
    flags = ConvBwdFlags(eb._FUSE_BN_ROWS, eb._DGRAD_BNSTATS, eb._SYNC_FUSED, eb._FUSE_BN_APPLY, eb._FUSE_BN_APPLY_L1, eb._LIN_WGRAD_AT)
    return plan_convstack_bwd(flags, sync_bn, B * T, F, hip.LINEAR_KERNELS, bool(L.a2s_linear_dgrad_eligible(B * T, 40 * F, CF, F)),
                              {c: bool(L.a2s_conv3x3_wgrad_bn_ranged_eligible(F, *c)) for c in CHANS[1:]})


def _expected_backward_calls(lin, layers, rows, F):
    """The helper calls _convstack_bwd makes for a plan, in order, with the deciding arguments (the Linear's weight gradient apart: its place moves)."""
    sync = lin.stats.startswith("sync")
    want = [("bn_bwd_sync" if sync else "bn_bwd", dict(partial=False, dx=True))]
    want.append(("gemm", dict(shape=(rows, 40 * F, CF))) if lin.dgrad == "gemm" else ("linear_dgrad_bnstats", dict(own=lin.dgrad == "own")))
    for lp in layers:
        stats = ("bn_bwd_sync" if lp.stats.startswith("sync") else "bn_bwd", dict(partial=lp.stats.endswith("partial"), dx=lp.form == "apply"))
        want.append(stats)
        if lp.form == "apply":
            want.append(("conv3x3_wgrad", dict(dy_absmax=lp.dy_range)))
        else:
            want.append(("conv3x3_wgrad_bn", dict(ranged=lp.form == "rows", dy=lp.form == "tiled" and lp.i > 1)))
        if lp.dgrad != "none":
            want.append(("conv3x3_dgrad", dict(below=lp.dgrad == "bnstats", dy_absmax=lp.dgrad_range, out_absmax=lp.out_range)))
    return want


def _seen_backward_calls(calls, rows, F):
    seen = []
    for name, a, _ in calls:
        if name == "bn_bwd":
            seen.append((name, dict(partial=a["partial"] is not None, dx=a["dx"] is not None)))
        elif name == "bn_bwd_sync":          # (the synchronised full form writes dx over g; from the partials it is statistics only)
            seen.append((name, dict(partial=a["partial"] is not None, dx=a["partial"] is None)))
        elif name == "gemm" and (a["M"], a["N"], a["K"]) == (rows, 40 * F, CF) and a["two_term"] is None and a["a_affine"] is None:
            seen.append((name, dict(shape=(rows, 40 * F, CF))))
        elif name == "linear_dgrad_bnstats":
            seen.append((name, dict(own=bool(a["own"]))))
        elif name == "conv3x3_wgrad":
            seen.append((name, dict(dy_absmax=a["dy_absmax"] is not None)))
        elif name == "conv3x3_wgrad_bn":
            seen.append((name, dict(ranged=a["ranged"] is not None, dy=a["dy"] is not None)))
        elif name == "conv3x3_dgrad":
            seen.append((name, dict(below=a["below"] is not None, dy_absmax=a["dy_absmax"] is not None, out_absmax=a["out_absmax"] is not None)))
    return seen


def _expected_counters(L, F, layers):
    """(forward, backward) increments of COUNTERS under the switches in force, from csrc/a2s_conv_rows.hip: the row kernels take conv2-conv4 and their
    data gradients where F % 4 == 0 and conv_rows has bit 0; the second generation (bit 1) counts its 20-channel-output launches (forward: conv2;
    backward: the data gradients of conv3 and conv2) and, with conv_rows_stage bit 0, its narrow-staging launches (forward: all three; backward:
    the data gradients of conv4 and conv3 with the statistics epilogue -- 20 -> 20 has no such form -- and every plain data gradient)."""
    rows_sw, stage = L.a2s_debug_get(b"conv_rows"), L.a2s_debug_get(b"conv_rows_stage")
    gen2 = F % 4 == 0 and (rows_sw & 1) and (rows_sw & 2)
    if not gen2:
        return dict.fromkeys(COUNTERS, 0), dict.fromkeys(COUNTERS, 0)
    narrow = bool(stage & 1)
    return (dict(conv_rows16_c20_launches=1, conv_rows_stage_launches=3 if narrow else 0),
            dict(conv_rows16_c20_launches=2, conv_rows_stage_launches=sum(lp.dgrad == "plain" or (lp.dgrad == "bnstats" and lp.i > 2) for lp in layers) if narrow else 0))


def _counters(L):
    return {k: L.a2s_debug_get(k.encode()) for k in COUNTERS}


# ------------------------------------------------------------------------------------------- driving one call
def _report(label, name, err, dev32, bar):
    from tests import test_gpu_ops
    test_gpu_ops._report(f"convstack_call {label} {name} (float32 oracle {dev32:.3e}, bar {bar:.3e})", err)


def _compare(label, views, dev32, project_bar, bad, F, scale=None):
    worst_ratio = 0.0
    for name, ref, got in views:
        assert torch.isfinite(got).all(), f"{label} {name}: non-finite"
        err = oracle.rel_err(got, ref, None if scale is None else scale[name])
        bar = max(project_bar, 3 * dev32[name])
        _report(label, name, err, dev32[name], bar)
        print(f"{label} {name}: {err:.3e}  float32 oracle {dev32[name]:.3e}  bar {bar:.3e}")
        worst_ratio = max(worst_ratio, err / bar)
        if not err <= bar:
            at, size = oracle.worst(got, ref)
            bad.append(f"{name}: {err:.3e} > {bar:.3e} (largest |got - ref| {size:.3e} at {oracle.where(name, at, F)})")
    return worst_ratio


def _forward(dev, i, F, training=True, sync_bn=False):
    from piano_a2s_amd import engine
    S = {k: v.clone().to(dev) for k, v in {**i["W"], **i["buffers"]}.items()}
    eng = engine.Engine(cfg(F), sync_bn=sync_bn)
    out, cs = eng.convstack(S, i["x"].to(dev), training, None if i["drop"] is None else i["drop"].to(dev))
    torch.cuda.synchronize()
    return S, eng, out, cs


def _backward(dev, i, S, eng, cs, B, T, F, prefill=None):
    from piano_a2s_amd import engine_bwd
    G = {k: (torch.zeros_like(S[k]) if prefill is None else prefill[k].to(dev)) for k in oracle.CONV_PARAMS}
    engine_bwd._convstack_bwd(eng, S, G, cs, i["d_out"].to(dev).clone(), B, T, F)
    torch.cuda.synchronize()                     # (the Linear's weight gradient may land from another stream)
    return {k: G[k].cpu() for k in oracle.CONV_PARAMS}


def _forward_tensors(out, cs):
    got = {"z": cs["z"].cpu(), "out": out.cpu()}
    for n, name in enumerate(("bn1", "bn2", "bn3", "bn4", "out_bn")):
        quad = cs["bn"][n] if n < 4 else cs["out_bn"]
        got.update({f"{name}.{k}": v.cpu() for k, v in zip(oracle.BN_PARTS, quad)})
    got.update({f"y{n + 1}": cs["y"][n].cpu() for n in range(4)})
    return got


def _check_ranges(label, cs):
    """The chain test's assertions on the operand ranges the forward saved: yabs is the exact maximum of the device's own y, abound the formula to
    2^-22 and not below the activations."""
    for n in range(4):
        y, (_, _, scale, shift) = cs["y"][n], cs["bn"][n]
        assert torch.equal(cs["yabs"][n], y.abs().amax(dim=(0, 1, 3))), f"{label}: yabs of layer {n + 1} is not max |y|"
        sc, sh = scale.double().view(1, 1, -1, 1), shift.double().view(1, 1, -1, 1)
        formula = float((scale.double().abs() * cs["yabs"][n].double() + shift.double().abs()).max())
        true_max = float(torch.relu(y.double() * sc + sh).max())
        bound = float(cs["abound"][n])
        assert abs(bound - formula) <= 2.0 ** -22 * formula, f"{label}: abound of layer {n + 1} is {bound!r}, the formula gives {formula!r}"
        assert bound * (1 + 2.0 ** -22) >= true_max, f"{label}: abound of layer {n + 1} ({bound!r}) lies below the activations ({true_max!r})"


def _call_and_check(dev, case, path="default", variant="plain", prefill=None, label=None):
    """One training call on `path`: plan, recorded calls and counters prove the path, every tensor holds its bar.  Returns a dict of what further
    assertions need (forward tensors, gradients, launch count, plan)."""
    from piano_a2s_amd import hip
    B, T, F = case
    rows = B * T
    i = inputs(B, T, F, variant)
    f64, _, _, dev32 = reference(B, T, F, variant)
    label = label or f"B{B}_T{T}_F{F}-{path}" + ("" if variant == "plain" else f"-{variant}")
    L = hip.lib()
    sync = bool(PATHS[path].get("sync_bn"))
    with _path(path), _one_rank_group(sync) as reduces, _record() as rec:
        lin, layers = _plan(L, path, B, T, F, sync)
        want_fwd, want_bwd = _expected_counters(L, F, layers)
        linear_kernels = hip.LINEAR_KERNELS
        lin_fwd_ok, lin_wgrad_ok = bool(L.a2s_linear_fwd_eligible(rows, CF, 40 * F, F)), bool(L.a2s_linear_wgrad_eligible(rows, CF, 40 * F, F))
        c0, n0 = _counters(L), L.a2s_launch_count()
        S, eng, out, cs = _forward(dev, i, F, sync_bn=sync)
        assert eng.sync_bn == sync
        c1, k1, r1 = _counters(L), rec.mark(), len(reduces)
        grads = _backward(dev, i, S, eng, cs, B, T, F, prefill)
        c2, n2, r2 = _counters(L), L.a2s_launch_count(), len(reduces)
    # ---- the path
    d1, d2 = {k: c1[k] - c0[k] for k in c0}, {k: c2[k] - c1[k] for k in c0}
    assert d1 == want_fwd, f"{label}: forward counters {d1}, expected {want_fwd}"
    assert d2 == want_bwd, f"{label}: backward counters {d2}, expected {want_bwd}"
    fwd_calls, bwd_calls = rec.calls[:k1], rec.calls[k1:]
    # (a training call of at most 64 rows takes the Linear in double, whatever the switches: Engine.convstack)
    names = [name for name, _, _ in fwd_calls]
    took = "f64" if "linear_forward_f64" in names else "generic" if "linear" in names else "own"
    assert names.count("linear_forward") + names.count("linear_forward_f64") == 1
    want_fwd_kernel = "f64" if rows <= 64 else "own" if linear_kernels and lin_fwd_ok else "generic"
    assert took == want_fwd_kernel, f"{label}: the Linear's forward took the {took} kernel, expected {want_fwd_kernel}"
    seen, want = _seen_backward_calls(bwd_calls, rows, F), _expected_backward_calls(lin, layers, rows, F)
    assert seen == want, f"{label}: the executor's calls {seen} are not the plan's {want}"
    wg = [ret for name, _, ret in bwd_calls if name == "linear_wgrad"]
    assert wg == [linear_kernels and lin_wgrad_ok], f"{label}: linear_wgrad returned {wg}"
    if sync:
        assert (r1, r2 - r1) == (5, 5), f"{label}: {r1} all-reduces in the forward, {r2 - r1} in the backward"
    if path == "default" and variant in ("plain", "dropout"):
        facts = FACTS[case]
        got_facts = dict(dgrad=lin.dgrad, forms=tuple(lp.form for lp in layers), stats=tuple(lp.stats for lp in layers),
                         lin_wgrad=wg[0], lin_fwd=took)
        assert got_facts == facts, f"{label}: this case is for {facts}, the call ran {got_facts}"
    # ---- forward
    got = _forward_tensors(out, cs)
    _check_ranges(label, cs)
    bad = []
    ratio = _compare(label, oracle.forward_views(f64, got), dev32, FWD_BAR, bad, F)
    after = {k: S[k].cpu() for k in oracle.BUFFERS}
    ratio = max(ratio, _compare(label, oracle.buffer_views(f64, after), dev32, STAT_BAR, bad, F))
    for k in oracle.BUFFERS:
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(f64["buffers"][k]), f"{label} {k}: {int(after[k])}, expected {int(f64['buffers'][k])}"
    bad_forward, bad = bad, []          # (asserted with the gradients at the end, so that a forward miss does not hide the backward's figures)
    # ---- the device's decisions
    masks, ambiguous = oracle.masks_from_saved([cs["y"][n] for n in range(4)], cs["bn"], cs["z"].view(B, T, CF), cs["out_bn"])
    keep = torch.ones(B, T, CF, dtype=torch.bool) if i["drop"] is None else (i["drop"] != 0).view(B, T, CF)
    assert torch.equal((got["out"].view(B, T, CF) > 0) & keep, masks[4] & keep), f"{label}: out > 0 is not the decision recomputed from z where the mask keeps"
    fl = flips(f64, masks, flip_margins(dev32))
    print(f"{label} flips per layer {[n for n, _ in fl]}; decisions a two-rounding evaluation would change {ambiguous}")
    for layer, (n, _) in enumerate(fl, start=1):
        _report(label, f"layer {layer} ReLU decisions that differ from the float64 oracle's", float(n), dev32[f"pre{layer}"], flip_margins(dev32)[layer - 1])
    far = [msg for _, msg in fl if msg]
    assert not far, f"{label}: a device ReLU decision differs from the oracle's beyond the flip margin -- the gradients are not compared: " + "; ".join(far)
    # ---- backward, under the device's decisions
    g64 = oracle.gradients(i["W"], i["buffers"], i["x"], i["drop"], True, i["d_out"], masks=masks)
    if prefill is None:
        views, scale = oracle.grad_views(g64, grads), None
    else:
        views = [(k, prefill[k].double() + g64[k], grads[k]) for k in oracle.CONV_PARAMS]
        scale = {k: float(g64[k].abs().max()) for k in oracle.CONV_PARAMS}
    ratio = max(ratio, _compare(label, views, dev32, GRAD_BAR, bad, F, scale))
    _report(label, "worst error / bar over the call", ratio, 0.0, 1.0)
    print(f"{label} launches {n2 - n0}, worst error / bar {ratio:.3f}")
    assert not bad_forward and not bad, f"{label}: forward: " + ("; ".join(bad_forward) or "within the bars") + " -- backward: " + ("; ".join(bad) or "within the bars")
    return dict(got=got, grads=grads, launches=n2 - n0, lin=lin, layers=layers, cs=cs, S=S, flips=[n for n, _ in fl])


_LAUNCHES = {}


def _launches(dev, path, case):
    """Launches of one call on `path` (run once per path and case, whichever test comes first)."""
    if (path, case) not in _LAUNCHES:
        _LAUNCHES[path, case] = _call_and_check(dev, case, path)["launches"]
    return _LAUNCHES[path, case]


@pytest.mark.parametrize("case", CASES, ids=[f"B{b}_T{t}_F{f}" for b, t, f in CASES])
def test_default_path_against_the_oracle(dev, case):
    """Every case on the switches' defaults; the plan each case is for (FACTS) is asserted."""
    _LAUNCHES["default", case] = _call_and_check(dev, case)["launches"]


SWITCHED = [(p, c) for p in PATHS if p != "default" for c in PATH_CASES] + [("conv_c1_fast0", (2, 3, 480))]


@pytest.mark.parametrize("path,case", SWITCHED, ids=[f"{p}-B{c[0]}_T{c[1]}_F{c[2]}" for p, c in SWITCHED])
def test_switched_path_against_the_oracle(dev, path, case):
    res = _call_and_check(dev, case, path)
    _LAUNCHES[path, case] = res["launches"]
    if path in COUNT_DIFFERS:
        other = COUNT_DIFFERS[path]
        assert res["launches"] != _launches(dev, other, case), f"{path}: {res['launches']} launches, as many as the path {other}"
    if path.startswith("wgrad_rows0"):
        assert all(lp.form != "rows" for lp in res["layers"])
    if path == "linear_kernels_off":
        assert res["lin"].dgrad != "own"
    if path == "sync_bn_unfused":
        assert all(lp.form == "apply" and lp.stats == "sync_own" for lp in res["layers"])


def test_eval_call_against_the_eval_oracle(dev):
    """training=False: the running statistics normalise, the buffers keep their bits, no statistics partials are allocated (the convolutions are
    handed none: Engine.convstack allocates them in training only, and a2s_bn_finalize is given a null pointer)."""
    from piano_a2s_amd import hip
    B, T, F = SMALL
    i = inputs(B, T, F)
    f64, _, _, dev32 = reference(B, T, F, "plain", False)
    seen = []
    real = hip.conv3x3_forward
    hip.conv3x3_forward = lambda *a, **kw: (seen.append(inspect.signature(real).bind(*a, **kw).arguments["partial"]), real(*a, **kw))[1]
    try:
        S, eng, out, cs = _forward(dev, i, F, training=False)
    finally:
        hip.conv3x3_forward = real
    assert seen == [None] * 4, "an eval call allocated statistics partials"
    for k in oracle.BUFFERS:
        assert torch.equal(S[k].cpu(), i["buffers"][k]), f"{k} changed in an eval call"
    label = f"B{B}_T{T}_F{F}-eval"
    _check_ranges(label, cs)
    bad = []
    _compare(label, oracle.forward_views(f64, _forward_tensors(out, cs)), dev32, FWD_BAR, bad, F)
    assert not bad, f"{label}: " + "; ".join(bad)


def test_training_call_with_a_dropout_mask(dev):
    """A seeded uint8 mask drops about a fifth of `out`: zero exactly there, the kept elements scaled by 1 / 0.8 (the oracle's `out`), and the
    backward takes the mask into the BatchNorm1d's backward."""
    B, T, F = SMALL
    drop = inputs(B, T, F, "dropout")["drop"]
    share = 1.0 - float(drop.float().mean())
    assert 0.15 < share < 0.25, share
    res = _call_and_check(dev, SMALL, "default", "dropout")
    out = res["got"]["out"].reshape(B * T, CF)
    assert float(out[drop == 0].abs().max()) == 0.0
    assert float(out[drop != 0].max()) > 0.0


@pytest.mark.parametrize("path", ["default", "linear_kernels_off"])
def test_parameter_gradients_accumulate(dev, path):
    """Every one of the 15 gradients is added to what G holds: pre-filled with seeded randn, G ends as pre-fill plus gradient, within the gradient
    bars measured against the gradient's own maximum."""
    W = inputs(*BIG)["W"]
    g = torch.Generator().manual_seed(99)
    prefill = {k: torch.randn(W[k].shape, generator=g) for k in oracle.CONV_PARAMS}
    _call_and_check(dev, BIG, path, prefill=prefill, label=f"B{BIG[0]}_T{BIG[1]}_F{BIG[2]}-{path}-prefilled")


@pytest.mark.parametrize("variant", ["gammas", "small"])
def test_other_magnitudes_on_the_own_linear_hand_off(dev, variant):
    """(2, 64, 128), default path -- the Linear's own data gradient hands its scalar max |da| to layer 4's a2s_conv3x3_wgrad_bn_ranged -- with every
    layer's range at another magnitude (CHAIN_GAMMAS, 2^+-3 spread per channel), and with x at 1e-3 and d_out at 1e-6 of their usual size."""
    res = _call_and_check(dev, BIG, "default", variant)
    assert res["lin"].dgrad == "own" and res["layers"][0].form == "rows"
