"""The host plan of the decoder with ground truth, pure (CPU tensors in, host data out; no device, no ctypes, no liba2s_hip.so): the coins, the executed
steps of every (bar, staff), the bar segments, the clip groups and, per decoder call, the row and clip bookkeeping the step kernels trust without
checking (include/a2s.h, a2s_note_dec_args).  engine.Engine.forward uploads what these functions return; train.TrainStep cuts the minibatch with them."""
import numpy as np
import torch

from .spec import EOS, PAD


def plan_note_steps(gt_rows, max_steps):
    """Host replay of the reference's loop bookkeeping for one (bar, staff) with ground truth
    (models.py:388-419): returns (steps executed, lengths per row).

    The loop breaks at the first t where every row has shown <eos> in gt[:, :t]; lengths[b] is overwritten by
    every <eos> seen at t < steps (so it ends as the LAST such position + 1), default max_steps.
    """
    B = gt_rows.shape[0]
    is_eos = gt_rows == EOS                                      # (B, max_steps) CPU bool
    first = torch.where(is_eos.any(1), is_eos.float().argmax(1), torch.full((B,), max_steps))
    steps = int(first.max()) + 1 if bool((first < max_steps).all()) else max_steps
    steps = min(steps, max_steps)
    idx = torch.arange(1, steps + 1, dtype=torch.long)
    last = (is_eos[:, :steps].long() * idx).amax(dim=1)          # last <eos> position + 1 among the executed steps, 0 = none
    lengths = torch.where(last > 0, last, torch.full((B,), max_steps, dtype=torch.long))
    return steps, lengths


def draw_plan(gt_cpu, bars, maxlen, rng, teacher_forcing_ratio):
    """The host plan of a forward pass with ground truth: executed steps of every (bar, staff) and EVERY coin of the reference's protocol, drawn in the
    reference's order (one per executed note step, upper then lower, then one per bar: models.py:404,289).  gt_cpu: (upper, lower, ...) host tensors
    (B, bars, len); the step counts are batch-wide maxima, so the clip order does not matter."""
    plan = []
    for bar in range(bars):
        p = {}
        for gi_idx in (0, 1):
            steps, _ = plan_note_steps(gt_cpu[gi_idx][:, bar, :], maxlen[gi_idx])
            p[gi_idx] = (steps, [rng.random() < teacher_forcing_ratio for _ in range(steps)])
        p["tf"] = rng.random() < teacher_forcing_ratio
        plan.append(p)
    return plan


def plan_segments(plan, bars, fuse, inference=False):
    """Bars decoded in one call each: consecutive bars whose predecessor's bar-level coin says "teacher-force" (at most 5 = A2S_ATTN_MAX_GROUPS)."""
    segments = [[0]]
    for bar in range(1, bars):
        if fuse and plan[bar - 1]["tf"] and not inference and len(segments[-1]) < 5:
            segments[-1].append(bar)
        else:
            segments.append([bar])
    return segments


def row_limits(gt_staff):
    """Decode steps every (clip, bar) row needs: the index of its last non-<pad> target + 1 (0: the row holds no target at all; a <pad> between
    real targets does not end it).  gt_staff: (B, bars, len) host tensor; returns (B, bars) int64."""
    idx = torch.arange(1, gt_staff.shape[-1] + 1)
    return ((gt_staff != PAD).long() * idx).amax(dim=-1)


def group_steps(plan, gt_group, maxlen):
    """Executed steps of every (bar, staff) call of ONE clip group: [{0: upper, 1: lower} per bar].  The loop of a (bar, staff) ends when every row
    OF THE GROUP has shown <eos> (a group with no full-length row does not run to the cap because another group has one), and never later than the
    plan's batch-wide count, whose coins it consumes.  gt_group: (upper, lower, ...) host targets of the group's clips, (clips, bars, len)."""
    return [{gi_idx: min(plan[bar][gi_idx][0], plan_note_steps(gt_group[gi_idx][:, bar, :], maxlen[gi_idx])[0]) for gi_idx in (0, 1)}
            for bar in range(len(plan))]


def segment_flags(plan, gsteps, seg, gi_idx):
    """One staff's decoder call over the bars `seg`: (steps, flags).  steps = the longest of the bars' step counts (group_steps); flags[t] = the
    teacher-forcing mask of step t, bit j = the plan's coin (global step index) of the j-th bar of the segment, 0 once that bar's loop has ended."""
    steps = max(gsteps[bar][gi_idx] for bar in seg)
    flags = [sum(int(t < gsteps[bar][gi_idx] and plan[bar][gi_idx][1][t]) << j for j, bar in enumerate(seg)) for t in range(steps)]
    return steps, flags


def segment_until(until_staff, gsteps, seg, gi_idx, b0, b1):
    """The until-matrix of one staff's decoder call over the bars `seg` and the clips [b0, b1): row_limits, bar-major (until_staff: (bars, B)), each
    bar clamped to its own step count -- the bar's loop ends there.  Returns (bars of the segment, clips)."""
    return torch.stack([until_staff[bar][b0:b1].clamp(max=gsteps[bar][gi_idx]) for bar in seg])


def _clip_plan(clip_until, n):
    """Clips sorted by the step their last row finishes at, latest first (stable); the inverse permutation; clips still running at each of n steps."""
    clips = clip_until.numel()
    order = torch.argsort(clip_until, descending=True, stable=True).to(torch.int32)
    rank = torch.empty_like(order)
    rank[order.long()] = torch.arange(clips, dtype=torch.int32)
    n_act = clips - torch.cumsum(torch.bincount(clip_until.long(), minlength=n + 1), 0)[:n]          # clips with until > t
    return order, rank, n_act


def staff_rows(until, n, tail_prefix=True, tail_rows=True, live_rows=True):
    """Row / clip bookkeeping of ONE decoder call of n launched steps (the row-plan fields of a2s_note_dec_args).  until: (bars of the segment,
    clips) int32, segment_until's; flat row = bar * clips + clip.  Returns host data only:
      until         flat (rows,) int32
      order, rank   (clips,) int32: the clips by the step their last row finishes at, latest first (stable), and the inverse permutation
      n_active      n ints: clips with an unfinished row at step t
      m_active      n ints: 1 + the largest clip POSITION with an unfinished row at step t, 0 = none  (None without tail_prefix)
      row_list      (rows,) int32: the rows by until, latest first (stable)                           (None without tail_rows)
      n_rows_active n ints: rows still running at step t                                               (None without tail_rows)
      live_idx      int32, ascending: step * rows + row of every (step, row) that still ran            (None without live_rows: O(steps x rows))
      live_steps    n
      n_clips       clips
      clip_steps    sum(n_active): the (clip, step) pairs whose keys / encoder outputs the call streams
    """
    clips = until.shape[1]
    clip_until = until.amax(dim=0)
    order, rank, n_act = _clip_plan(clip_until, n)
    m_act = row_list = n_rows = live_idx = None
    if tail_prefix:
        # (the per-step products of the tail run on that prefix of every fused bar only; plan_clip_groups puts the clips with the longest rows first)
        last = torch.zeros(n + 1, dtype=torch.long)
        cu = clip_until.long().clamp(max=n)
        last.scatter_reduce_(0, cu, torch.arange(1, clips + 1), reduce="amax")                       # last[u] = 1 + max position with until == u
        m_act = torch.flip(torch.cummax(torch.flip(last, [0]), 0)[0], [0])[1:n + 1].tolist()         # max over until > t
    uflat = until.reshape(-1)
    if tail_rows:
        row_list = torch.argsort(uflat, descending=True, stable=True).to(torch.int32)
        rcnt = torch.bincount(uflat.long().clamp(max=n), minlength=n + 1)
        n_rows = (uflat.numel() - torch.cumsum(rcnt, 0)[:n]).tolist()                                # rows with until > t
    if live_rows:
        live_idx = (torch.arange(n).unsqueeze(1) < uflat.unsqueeze(0)).reshape(-1).nonzero().squeeze(1).to(torch.int32)
    return dict(until=uflat, order=order, rank=rank, live_idx=live_idx, live_steps=n, n_active=n_act.tolist(), n_clips=clips, m_active=m_act,
                row_list=row_list, n_rows_active=n_rows, clip_steps=int(n_act.sum()))


def pair_rows(until_up, until_lo, n, few_rows):
    """Clip bookkeeping of BOTH staves of a segment issued by one loop of n steps (a2s_note_decoder_fwd_pair): order / rank / n_active as in
    staff_rows, over the rows of both until-matrices together.  shared_clip_steps = the (clip, step) pairs whose encoder outputs ONE pass serves
    for both staves: steps at which each staff has more than few_rows rows still running (the launch-per-step loop; few_rows = what the few-row
    kernels take), clips with an unfinished row of each staff."""
    order, rank, n_act = _clip_plan(torch.cat([until_up, until_lo]).amax(dim=0), n)
    t_ = torch.arange(n).unsqueeze(1)
    rows_live = [(u.reshape(1, -1) > t_).sum(1) for u in (until_up, until_lo)]
    clip_live = [u.amax(dim=0).unsqueeze(0) > t_ for u in (until_up, until_lo)]
    joint = (rows_live[0] > few_rows) & (rows_live[1] > few_rows)
    return dict(order=order, rank=rank, n_active=n_act.tolist(), shared_clip_steps=int(((clip_live[0] & clip_live[1]).sum(1) * joint).sum()))


def plan_clip_groups(until_up, until_lo, max_tail_frac=0.5, min_gain=0.08, step_cost=150.0, jump=1.3, max_candidates=8):
    """Cut a minibatch into [ordinary clips | long clips] for Engine.forward's clip groups.

    until_up / until_lo: (B, bars) int arrays, decode steps each (clip, bar) row needs (last real target + 1).  Cost model of a group
    of clips, in units of one clip's attention pass (~0.7 us on MI355X): a decode step costs max(step_cost, rows still active) --
    bandwidth-bound while many rows are active, a latency floor (~100 us of dependent small kernels) once only a few long rows
    remain -- summed over the steps of the longer staff of every bar.  Two groups run CONCURRENTLY but share the HBM, so a cut costs
    max(cost of either group, attention work of both).  Candidate cuts: the places where the clips' longest rows, sorted, jump by
    `jump`x.  The best cut is taken if it beats the uncut minibatch by min_gain.  Returns (order, n_main): `order` = clip permutation
    (ordinary clips first, sorted by their longest row, longest first; the long clips in their original order), n_main = size of the
    first group (== B: do not split)."""
    up, lo = np.asarray(until_up, dtype=np.int64), np.asarray(until_lo, dtype=np.int64)
    B = up.shape[0]
    ident = np.arange(B)
    if B < 4:
        return ident, B

    def cost(sel):
        total, work = 0.0, 0.0
        for bar in range(up.shape[1]):
            u, l = up[sel, bar], lo[sel, bar]
            n = int(max(u.max(), l.max()))
            act = np.zeros(n, dtype=np.float64)
            for v in (u, l):
                act += len(v) - np.cumsum(np.bincount(v, minlength=n + 1))[:n]         # rows with until > t
            total += np.maximum(act, step_cost).sum()
            work += act.sum()
        return total, work

    longest = np.maximum(up.max(1), lo.max(1))
    by_len = np.argsort(-longest, kind="stable")                 # longest clips first
    srt = longest[by_len].astype(np.float64)
    kmax = max(1, int(B * max_tail_frac))
    ratio = srt[:kmax] / np.maximum(srt[1:kmax + 1], 1.0)        # jump between the k-th longest clip and the next
    cands = [int(k) + 1 for k in np.argsort(-ratio, kind="stable")[:max_candidates] if ratio[k] >= jump]
    if not cands:
        return ident, B
    whole, _ = cost(ident)
    best_k, best = None, (1.0 - min_gain) * whole
    for k in cands:
        ct, wt = cost(by_len[:k])
        cm, wm = cost(by_len[k:])
        c = max(ct, cm, wt + wm)
        if c < best:
            best_k, best = k, c
    if best_k is None:
        return ident, B
    # inside the ordinary group the clips with the longest rows come first (by_len is a stable descending sort): late in a decoder call
    # only a prefix of the clips is still running (staff_rows: m_active); the long clips keep their original order
    return np.concatenate([by_len[best_k:], np.sort(by_len[:best_k])]), B - best_k


def split_long_group(long_ids, until_up, until_lo, segments, min_gain=0.1):
    """Round 5.  The long-clip group's decode chain is, per bar SEGMENT of the step, as long as the longest row ANY of its clips has there -- typically a
    full-length (398-step) upper bar in every segment, although each clip holds only one such bar.  Cut it by where the clips' longest bars lie:
    sub-group A = clips whose longest upper bar is in segments 0..k, sub-group B = the rest; each then runs 398 steps only in "its" segments.  The two
    sub-groups get one stream each (engine.group_stream) and decode their staves one after the other, so a sub-group's chain is the SUM of its
    staves' steps per segment, against the MAXIMUM for the single group (staves side by side).  Returns (A, B) -- lists of clip ids -- for the
    best k when max(chain A, chain B) < (1 - min_gain) x the single group's chain, else None.  Loss, gradients and update do not depend on the
    grouping (clip groups are independent: Engine.forward)."""
    long_ids = list(long_ids)
    if len(long_ids) < 2 or len(segments) < 2:
        return None
    up, lo = np.asarray(until_up), np.asarray(until_lo)

    def chain(ids, sequential):
        total = 0
        for seg in segments:
            u, l = int(up[np.ix_(ids, seg)].max()), int(lo[np.ix_(ids, seg)].max())
            total += (u + l) if sequential else max(u, l)
        return total
    seg_of_bar = {bar: si for si, seg in enumerate(segments) for bar in seg}
    where = [seg_of_bar[int(up[c].argmax())] for c in long_ids]
    single = chain(long_ids, False)
    best = None
    for k in range(len(segments) - 1):
        a = [c for c, w in zip(long_ids, where) if w <= k]
        b = [c for c, w in zip(long_ids, where) if w > k]
        if not a or not b:
            continue
        m = max(chain(a, True), chain(b, True))
        if best is None or m < best[0]:
            best = (m, a, b)
    if best is not None and best[0] < (1.0 - min_gain) * single:
        return best[1], best[2]
    return None


def plan_step_groups(gt_host, bars, max_length, rng, teacher_forcing_ratio, group_plan=None, long_subgroups=True, cut=None):
    """The host's clip-group plan of one step, from the targets alone: gt_host = (upper, lower, ...) host tensors (B, bars, len).  Returns (order,
    group_cuts, host_plan): the clip permutation, the contiguous clip ranges of the groups in that order -- [ordinary | long] or, when the long
    clips' longest bars lie in different bar segments of THIS step's coins, [ordinary | long A | long B] (split_long_group) -- and the coins if
    they had to be drawn for that (draw_plan: the reference's draw order; Engine.forward then takes them as host_plan), else None.
    cut: the function that cuts [ordinary | long], plan_clip_groups unless given (train.TrainStep passes train.plan_clip_groups, the name tests and
    tools wrap).  TrainStep._step calls it; tests/golden/make_golden.py uses it to choose fixtures that exercise the three-group path."""
    until_u, until_l = row_limits(gt_host[0]).numpy(), row_limits(gt_host[1]).numpy()
    order, n_main = (cut or plan_clip_groups)(until_u, until_l, **(group_plan or {}))
    B = gt_host[0].shape[0]
    group_cuts, host_plan = [(0, n_main), (n_main, B)], None
    if n_main < B and long_subgroups:
        # the coins of the step are drawn HERE, in the reference's order: the cut looks at the bar segments
        host_plan = draw_plan(gt_host, bars, max_length, rng, teacher_forcing_ratio)
        sub = split_long_group(order[n_main:].tolist(), until_u, until_l, plan_segments(host_plan, bars, True))
        if sub is not None:
            order = np.concatenate([order[:n_main], np.asarray(sub[0], dtype=order.dtype), np.asarray(sub[1], dtype=order.dtype)])
            group_cuts = [(0, n_main), (n_main, n_main + len(sub[0])), (n_main + len(sub[0]), B)]
    return order, group_cuts, host_plan
