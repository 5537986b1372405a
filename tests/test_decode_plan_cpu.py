"""The decoder's host plan (piano_a2s_amd.decode_plan, no GPU): the row and clip bookkeeping of a decoder call against literal definitions written
with loops from the field descriptions of a2s_note_dec_args (include/a2s.h), the pair loop's joint clip order and shared (clip, step) count, the
per-group step counts and teacher-forcing masks, the row limits -- and that the module stays importable without the HIP library."""
import os
import random
import subprocess
import sys

import pytest
import torch

from piano_a2s_amd import decode_plan, spec, synthetic
from piano_a2s_amd.spec import PAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 3), (2, 4), (5, 2), (3, 7))          # (bars of the segment, clips)


def test_module_is_pure_host_code():
    code = ("import sys, piano_a2s_amd.decode_plan; "
            "bad = [m for m in ('piano_a2s_amd.hip', 'piano_a2s_amd.abi', 'piano_a2s_amd.engine', 'piano_a2s_amd.train') if m in sys.modules]; "
            "assert not bad, bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- the literal definitions: U[k][c] = until of bar k of the segment, clip c; flat row r = k * clips + c; n steps
def _clip_defs(clip_until, n):
    clips = len(clip_until)
    order = sorted(range(clips), key=lambda c: -clip_until[c])          # (sorted is stable: ties in clip order)
    rank = [0] * clips
    for pos, c in enumerate(order):
        rank[c] = pos
    n_active = [sum(1 for c in range(clips) if clip_until[c] > t) for t in range(n)]
    return order, rank, n_active


def _staff_defs(U, n):
    nb, clips = len(U), len(U[0])
    clip_until = [max(U[k][c] for k in range(nb)) for c in range(clips)]
    order, rank, n_active = _clip_defs(clip_until, n)
    m_active = [max([c + 1 for c in range(clips) if clip_until[c] > t], default=0) for t in range(n)]
    flat = [U[k][c] for k in range(nb) for c in range(clips)]
    rows = len(flat)
    row_list = sorted(range(rows), key=lambda r: -flat[r])
    n_rows_active = [sum(1 for r in range(rows) if flat[r] > t) for t in range(n)]
    live_idx = [t * rows + r for t in range(n) for r in range(rows) if flat[r] > t]
    return dict(until=flat, order=order, rank=rank, n_active=n_active, m_active=m_active, row_list=row_list, n_rows_active=n_rows_active,
                live_idx=live_idx, live_steps=n, n_clips=clips, clip_steps=sum(n_active))


def _until_cases(nb, clips, seed):
    """(U, n) cases for one shape: random untils in 0..9 against n below, at and above them (n = 0 included), a clip finished at step 0 in
    every bar, all rows equal, and untils above n clamped the way the caller does."""
    g = torch.Generator().manual_seed(seed)
    cases = []
    for n in (0, 1, 4, 9, 12):
        cases.append((torch.randint(0, 10, (nb, clips), generator=g, dtype=torch.int32).clamp(max=n), n))
    dead = torch.randint(1, 10, (nb, clips), generator=g, dtype=torch.int32)
    dead[:, clips // 2] = 0
    cases.append((dead, 9))
    for v, n in ((0, 0), (0, 3), (5, 5), (3, 7)):
        cases.append((torch.full((nb, clips), v, dtype=torch.int32), n))
    raw = torch.randint(0, 10, (nb, clips), generator=g, dtype=torch.int32)           # until above n before clamping
    assert int(raw.max()) > 5 or nb * clips == 1
    cases.append((raw.clamp(max=5), 5))
    return cases


def _as_lists(p):
    return {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in p.items()}


@pytest.mark.parametrize("nb,clips", SHAPES)
def test_staff_rows_are_the_field_definitions(nb, clips):
    for U, n in _until_cases(nb, clips, 17 * nb + clips):
        got = decode_plan.staff_rows(U.clone(), n)
        want = _staff_defs(U.tolist(), n)
        assert _as_lists(got) == want, (U.tolist(), n)
        # what is uploaded is int32, what stays on the host are Python ints
        assert all(got[k].dtype == torch.int32 for k in ("until", "order", "rank", "row_list", "live_idx"))
        assert all(type(x) is int for k in ("n_active", "m_active", "n_rows_active") for x in got[k]) and type(got["clip_steps"]) is int
        assert all(len(got[k]) == n for k in ("n_active", "m_active", "n_rows_active"))


@pytest.mark.parametrize("nb,clips", ((2, 4), (3, 7)))
def test_staff_rows_flags_drop_only_their_part(nb, clips):
    parts = {"tail_prefix": ("m_active",), "tail_rows": ("row_list", "n_rows_active"), "live_rows": ("live_idx",)}
    for U, n in _until_cases(nb, clips, 5):
        full = _as_lists(decode_plan.staff_rows(U, n))
        for flag, keys in parts.items():
            got = _as_lists(decode_plan.staff_rows(U, n, **{flag: False}))
            assert all(got[k] is None for k in keys), flag
            assert {k: v for k, v in got.items() if k not in keys} == {k: v for k, v in full.items() if k not in keys}, flag
        none = _as_lists(decode_plan.staff_rows(U, n, False, False, False))
        gone = [k for keys in parts.values() for k in keys]
        assert all(none[k] is None for k in gone) and {k: v for k, v in none.items() if k not in gone} == {k: v for k, v in full.items() if k not in gone}


@pytest.mark.parametrize("nb,clips", SHAPES)
def test_pair_rows_are_the_field_definitions(nb, clips):
    ups, los = _until_cases(nb, clips, 31 * nb + clips), _until_cases(nb, clips, 7 * nb + 3 * clips)
    for (Uu, nu), (Ul, nl) in zip(ups, los[1:] + los[:1]):            # (shifted: the two staves run different numbers of steps)
        n = max(nu, nl)
        uu, ul = Uu.tolist(), Ul.tolist()
        clip_until = [max(max(uu[k][c], ul[k][c]) for k in range(nb)) for c in range(clips)]
        order, rank, n_active = _clip_defs(clip_until, n)
        for few_rows in (0, 1, nb * clips):
            shared = 0
            for t in range(n):
                rows_live = [sum(1 for k in range(nb) for c in range(clips) if u[k][c] > t) for u in (uu, ul)]
                if rows_live[0] > few_rows and rows_live[1] > few_rows:
                    shared += sum(1 for c in range(clips) if any(uu[k][c] > t for k in range(nb)) and any(ul[k][c] > t for k in range(nb)))
            got = decode_plan.pair_rows(Uu, Ul, n, few_rows)
            assert _as_lists(got) == dict(order=order, rank=rank, n_active=n_active, shared_clip_steps=shared), (uu, ul, n, few_rows)
            assert got["order"].dtype == torch.int32 and got["rank"].dtype == torch.int32 and type(got["shared_clip_steps"]) is int
            if few_rows == nb * clips:
                assert shared == 0


def test_row_limits():
    g = torch.Generator().manual_seed(2)
    gt = torch.randint(0, PAD, (4, 3, 9), generator=g)
    gt[torch.rand((4, 3, 9), generator=g) < 0.4] = PAD
    gt[0, 0, :] = PAD                                            # no target at all
    gt[1, 1, :] = torch.tensor([5, PAD, PAD, 7, 8, PAD, PAD, PAD, PAD])       # <pad> in the middle: the last real target counts
    gt[2, 2, -1] = 3                                             # a full-length row
    got = decode_plan.row_limits(gt)
    want = [[max([t + 1 for t in range(9) if int(gt[b, bar, t]) != PAD], default=0) for bar in range(3)] for b in range(4)]
    assert got.tolist() == want and got.shape == (4, 3)
    assert want[0][0] == 0 and want[1][1] == 5 and want[2][2] == 9


def test_group_steps_and_flag_masks():
    cfg = spec.default_cfg(max_length=(14, 9))
    batch = synthetic.make_batch(6, cfg, 3, frames=9, upper_range=(1, 14), lower_range=(1, 9), full_tail=0.2)
    gt = (batch[3], batch[5], batch[4], batch[6])
    bars, maxlen = cfg["max_bars"], cfg["max_length"]
    assert bars == 5
    plan = decode_plan.draw_plan(gt, bars, maxlen, random.Random(5), 0.7)
    shorter = 0
    for b0, b1 in ((0, 4), (4, 6)):
        gt_g = tuple(t[b0:b1] for t in gt)
        gsteps = decode_plan.group_steps(plan, gt_g, maxlen)
        assert len(gsteps) == bars
        for bar in range(bars):
            for gi in (0, 1):
                own = decode_plan.plan_note_steps(gt_g[gi][:, bar, :], maxlen[gi])[0]
                assert gsteps[bar][gi] == min(plan[bar][gi][0], own)
                shorter += gsteps[bar][gi] < plan[bar][gi][0]
        for segments in ([[0, 1, 2, 3, 4]], [[0], [1, 2], [3, 4]]):          # (one 5-bar segment; one-bar and two-bar segments)
            for seg in segments:
                for gi in (0, 1):
                    steps, flags = decode_plan.segment_flags(plan, gsteps, seg, gi)
                    assert steps == max(gsteps[bar][gi] for bar in seg) and len(flags) == steps
                    for t in range(steps):
                        for j, bar in enumerate(seg):
                            assert (flags[t] >> j) & 1 == int(t < gsteps[bar][gi] and plan[bar][gi][1][t]), (seg, gi, t, j)
                        assert flags[t] >> len(seg) == 0
    assert shorter > 0, "some call of a group must end before the batch-wide count, or the min() is not exercised"


def test_segment_until_clamps_each_bar_to_its_own_steps():
    until_staff = torch.tensor([[9, 2, 0, 5], [3, 3, 8, 1], [7, 7, 7, 7]], dtype=torch.int32)      # (bars, B)
    gsteps = [{0: 4, 1: 9}, {0: 9, 1: 9}, {0: 0, 1: 9}]
    got = decode_plan.segment_until(until_staff, gsteps, [0, 2], 0, 1, 4)
    assert got.tolist() == [[2, 0, 4], [0, 0, 0]] and got.dtype == torch.int32
    assert decode_plan.segment_until(until_staff, gsteps, [1], 1, 0, 4).tolist() == [[3, 3, 8, 1]]
