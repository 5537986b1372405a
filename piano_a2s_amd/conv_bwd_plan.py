"""The host plan of the ConvStack's backward pass, pure (host data in, host data out: no device, no ctypes, no liba2s_hip.so): which kernel forms every
layer's BatchNorm backward, weight gradient and data gradient take, where the BatchNorm statistics come from, which launch produces an operand range
or statistics partials and which one consumes them, and where the 19200 -> 256 Linear's weight gradient is issued.  engine_bwd._convstack_bwd reads its
module switches into a ConvBwdFlags, asks the library the two eligibility questions, and walks the plan; it decides nothing itself.

The chain, output to input: BatchNorm1d (+ ReLU, dropout) over the Linear's output -> Linear -> layers 4, 3, 2, 1, each BatchNorm2d then 3x3 convolution.
The gradient entering a layer may carry two things its producer reduced while it wrote the tensor: the BatchNorm-backward statistics PARTIALS of the
layer (no statistics pass then) and a RANGE, max |g| as a device scalar (from the Linear) or per channel (from a data-gradient convolution), by which
the row-streaming weight gradient scales its fp16 operand.  The kernels trust both without checking: a range handed to the wrong layer gives finite,
wrong gradients (tests/test_conv_bwd_plan_cpu.py holds the wiring, tests/test_gpu_operand_ranges.py the numbers)."""
from collections import namedtuple

CHANS = ((1, 20), (20, 20), (20, 40), (40, 40))          # (in, out) channels of conv1 .. conv4
LIN_WGRAD_PLACES = ("before", "beside", 4, 3, 2)


class ConvBwdFlags(namedtuple("ConvBwdFlags", "fuse_bn_rows dgrad_bnstats sync_fused fuse_bn_apply fuse_bn_apply_l1 lin_wgrad_at",
                              defaults=(True, True, True, False, True, "before"))):
    """The switches of engine_bwd (module attributes there, read once per call), with their defaults.
    fuse_bn_rows: BatchNorm-backward apply inside the row-streaming weight gradient's staging waves (A2S_FUSE_BN_ROWS=0: a tensor pass of its own).
    dgrad_bnstats: the statistics of the layer below in the epilogue of the data gradient (the Linear's included).
    sync_fused: synchronised BatchNorm keeps these fused paths (one small all-reduce per layer); False: separate statistics + apply passes.
    fuse_bn_apply / fuse_bn_apply_l1: the apply inside the TILED weight gradient a2s_conv3x3_wgrad_bn (dy = scale (g' - c1 - xhat c2) formed while the
    kernel stages its dy operand), for every layer (parity-tested, slower: the extra operand pushes conv3x3_wgrad<40> from 202 to 281 registers) / for
    conv1, whose weight gradient is a kernel of its own and whose input gradient nothing else reads (one pass over (g, y) instead of two).
    lin_wgrad_at: where the Linear's weight gradient (reads y4 once, 10-11 ms, only the optimizer waits for it) is issued: "before" the data gradient on
    the main stream; "beside" it on the weight-gradient stream; 4 / 3 / 2: on that stream at the top of that layer's turn.  Step time in that order:
    454.6, 454.5, 456.9, 456.3, 463.3 ms (profiles/r06_ab_switches.txt, r06_ab_lin_wgrad_placement.txt): no placement of this launch moves the step;
    the simplest is the default."""


class LinearPlan(namedtuple("LinearPlan", "stats absmax_after dgrad wgrad_at join_side")):
    """stats: statistics source of the BatchNorm1d above the Linear (always the full form: "own" / "sync_own"); absmax_after: max |dz| by a pass of its own
    (the synchronised apply does not reduce it).  dgrad: "own" (csrc/a2s_linear.hip: partials and max |da|), "generic" (two-term GEMM tiles with the
    statistics epilogue: partials) or "gemm" (neither).  wgrad_at: see ConvBwdFlags.lin_wgrad_at; join_side: the weight gradient ran on the
    weight-gradient stream, so the main stream waits for that stream at the end of the ConvStack backward."""


class LayerPlan(namedtuple("LayerPlan", "i ci co dy_range form stats absmax_after lin_wgrad dgrad dgrad_range out_range")):
    """Layer i with channels ci -> co.
    dy_range: the layer owns a device scalar max |dy|, zeroed by the executor and reduced by the kernel that writes dy: the two-term fp16 kernels that read dy scale
    it by the matching power of two (gradients would otherwise sit in fp16's subnormal range).
    form: how BatchNorm backward and weight gradient are launched.
      "rows"  -- statistics only, then a2s_conv3x3_wgrad_bn_ranged: dy = scale (g' - c1 - xhat c2) is formed by the STAGING waves of the row-streaming
                 kernel (they wait 40-57 % of their time for the multiply waves) and written once, over g in place (every element is read and written
                 by the same thread), with its range: one pass over (g, y) less than "apply".  Needs partials and a range with the incoming gradient.
      "apply" -- the full BatchNorm backward over g in place, which writes the range (absmax_after: the synchronised one does not; a2s_absmax does),
                 then a2s_conv3x3_wgrad_ranged.
      "tiled" -- statistics only, then a2s_conv3x3_wgrad_bn, which forms dy while it stages its operand and writes it to a fresh tensor; no range.
                 Layer 1 has no data gradient, so its dy is never written: one pass over (g, y) instead of apply (read 2, write 1) + read 1.
    stats: see stats_source.  lin_wgrad: the Linear's weight gradient is issued on the weight-gradient stream before anything of this layer.
    dgrad: "bnstats" (a2s_conv3x3_dgrad_bnstats_ranged: partials for the layer below in its epilogue; dgrad_range: it is given the layer's max |dy|;
    out_range: it writes the per-channel range of what it produces), "plain" (a2s_conv3x3, flip = 1: nothing for the layer below) or "none" (layer 1)."""


def stats_source(sync_bn, stats_only, has_partial):
    """Where a BatchNorm backward's statistics come from.  "partial": the producer's partials (a2s_bn_bwd_from_partial_amax).  "sync_partial": the
    partials -> this rank's sums -> one all-reduce -> the means from the global sums (statistics only: a2s_bn_bwd_sums_from_partial,
    a2s_bn_bwd_c12_from_sums).  "own": a pass over (g, x) (a2s_bn_bwd_amax).  "sync_own": a2s_bn_bwd_stats, one all-reduce, a2s_bn_bwd_apply (always
    the full form: the synchronised full form has no use for partials).  Synchronised, statistics only and no partials: no kernel does that."""
    if has_partial and not sync_bn:
        return "partial"
    if has_partial and stats_only:
        return "sync_partial"
    if sync_bn and stats_only:
        raise ValueError("synchronised BatchNorm backward, statistics only, without the producer's partials: not a plan")
    return "sync_own" if sync_bn else "own"


def plan_convstack_bwd(flags, sync_bn, rows, F, linear_kernels, linear_dgrad_eligible, ranged_eligible):
    """rows = B * T; linear_kernels: hip.LINEAR_KERNELS; linear_dgrad_eligible: the library's answer for this shape; ranged_eligible: its answer for
    a2s_conv3x3_wgrad_bn_ranged, one bool or {(ci, co): bool} for conv2 .. conv4.  Returns (LinearPlan, the LayerPlan of layers 4, 3, 2, 1)."""
    if isinstance(flags.lin_wgrad_at, bool) or flags.lin_wgrad_at not in LIN_WGRAD_PLACES:
        raise ValueError(f"lin_wgrad_at = {flags.lin_wgrad_at!r}: expected one of {LIN_WGRAD_PLACES}")
    fused_ok = not sync_bn or flags.sync_fused
    stats = flags.dgrad_bnstats and fused_ok
    epilogue = stats and F >= 128 and F % 4 == 0 and rows > 64          # (the statistics epilogue lives in the 128-row GEMM tile)
    dgrad = ("own" if linear_kernels and linear_dgrad_eligible else "generic") if epilogue else "gemm"
    linear = LinearPlan(stats_source(sync_bn, False, False), sync_bn, dgrad, flags.lin_wgrad_at, flags.lin_wgrad_at != "before")
    partial, amax = dgrad != "gemm", dgrad == "own"          # what the gradient entering the next layer carries
    layers = []
    for i in (4, 3, 2, 1):
        ci, co = CHANS[i - 1]
        eligible = ranged_eligible[(ci, co)] if isinstance(ranged_eligible, dict) and i > 1 else ranged_eligible
        rows_form = flags.fuse_bn_rows and fused_ok and i > 1 and partial and amax and eligible
        tiled = not sync_bn and (flags.fuse_bn_apply or (i == 1 and flags.fuse_bn_apply_l1))
        form = "rows" if rows_form else "tiled" if tiled else "apply"
        dy_range = i > 1 and fused_ok
        out_range = i > 2 and stats and flags.fuse_bn_rows
        layers.append(LayerPlan(i, ci, co, dy_range, form, stats_source(sync_bn, form != "apply", partial), form == "apply" and sync_bn and dy_range,
                                flags.lin_wgrad_at == i, "none" if i == 1 else "bnstats" if stats else "plain",
                                # (the range is withheld under fuse_bn_apply whatever the form: "tiled" writes none)
                                i > 1 and stats and dy_range and not flags.fuse_bn_apply, out_range))
        partial, amax = stats, out_range
    return linear, tuple(layers)
