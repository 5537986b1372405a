"""ctypes binding of liba2s_hip.so (include/a2s.h).  There is NO fallback: if the library is missing or a
call fails, this raises -- the product path never silently runs anything else."""
import ctypes as C
import os
import threading

import numpy as np
import torch

from .abi import PROTOTYPES, STRUCTS, A2SError          # the ABI as include/a2s.h declares it; the package's one error type
from .build import LIB

LIB = os.environ.get("A2S_LIB", LIB)          # A/B measurements against an older build of the library

# the argument blocks as include/a2s.h declares them (abi.py; lib() types the prototypes from it too): nothing of the ABI is restated here
NoteDecArgs, NoteDecBwdArgs, BeamArgs, AlignArgs = (STRUCTS[n] for n in ("a2s_note_dec_args", "a2s_note_dec_bwd_args", "a2s_beam_args", "a2s_align_args"))
_lib = None


def set_row_plan(a, active):
    """The row plan of a decoder call (the eight fields a2s_note_dec_args and a2s_note_dec_bwd_args share) from `active` = dict(until, order, rank:
    device int32 tensors; n_active: C int array per step; n_clips; optional m_active: C int array, row_list: device int32 + n_rows_active: C int
    array), or from None: plain rows, nothing fused, nothing skipped."""
    active = active or {}
    for field, key in (("clip_order", "order"), ("clip_rank", "rank"), ("row_until", "until"), ("row_list", "row_list")):
        setattr(a, field, active[key].data_ptr() if active.get(key) is not None else None)
    for field, key in (("n_active", "n_active"), ("m_active", "m_active"), ("n_rows_active", "n_rows_active")):
        host = active.get(key) if (key != "n_rows_active" or active.get("row_list") is not None) else None
        setattr(a, field, C.cast(host, C.c_void_p).value if host is not None else None)
    a.n_clips = active.get("n_clips", 0)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise A2SError(f"HIP extension not built: {LIB} is missing (run `python __graft_entry__.py build`). "
                           "There is no CPU fallback for the transcription hot path.")
        # A2S_ARITH: the arithmetic of the dense contractions -- "f16x2" (default: two exact fp16 terms per fp32 operand, three
        # products), "bf16x3" (rounds 1-2: three bf16 terms, six products) or "f32" (fp32-input matrix instructions / vector FMAs); per-kernel keys:
        # a2s_debug_set("conv_f16x2" | "wgrad_f16x2" | "gemm_f16x2" | "conv_bf16x3" | "gemm_bf16x3" | "wgrad_bf16x3", n)
        arith = os.environ.get("A2S_ARITH", "f16x2")
        if arith not in ("f16x2", "bf16x3", "f32"):
            raise A2SError(f"A2S_ARITH={arith!r}: expected f16x2, bf16x3 or f32")
        L = C.CDLL(LIB)
        for name, restype, argtypes in PROTOTYPES:          # every prototype the library exports is typed once, here: calls take plain Python numbers
            fn = getattr(L, name, None)                  # (a build from before an entry point lacks it and leaves it unbound: its callers test hasattr)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        # the library has read the variables that override a switch's default itself (csrc/a2s_switches.h: the documented fallbacks of INTEGRATION.md)
        # (a build from before that call -- A2S_LIB, tools/lib_ab.sh -- reads them lazily and has nothing to report)
        if hasattr(L, "a2s_env_check") and L.a2s_env_check() != 0:
            raise A2SError(L.a2s_last_error().decode())
        if arith != "f16x2":
            for key in (b"conv_f16x2", b"wgrad_f16x2", b"gemm_f16x2"):
                L.a2s_debug_set(key, 0)
        if arith == "f32":
            for key in (b"conv_bf16x3", b"gemm_bf16x3", b"wgrad_bf16x3"):
                L.a2s_debug_set(key, 0)
        _lib = L          # published only once it is fully configured: a failed first call leaves nothing half-made behind
    return _lib


# the 19200 -> 256 Linear on the kernels of csrc/a2s_linear.hip (A2S_LINEAR_KERNELS=0: the generic two-term GEMM tiles; bench.py times both)
LINEAR_KERNELS = os.environ.get("A2S_LINEAR_KERNELS", "1") != "0"

_ABORT_LATCH = {}
PERSIST_ABORTS = 0          # persistent launches of this process that gave up a bounded wait (observed through the latch)


def abort_latch(device):
    """The device word the persistent kernels OR a bit into when one of their bounded waits gives up (a2s_persist_abort_latch): allocated
    and registered on first use; one process drives one GPU, so the library keeps one pointer."""
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    t = _ABORT_LATCH.get(idx)
    if t is None:
        t = _ABORT_LATCH[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
        _ABORT_LATCH["registered"] = None
    if _ABORT_LATCH.get("registered") != idx:
        check(lib().a2s_persist_abort_latch(_p(t)), "a2s_persist_abort_latch")
        _ABORT_LATCH["registered"] = idx
    return t


_LATCH_READS = {}         # device index -> [pinned host word, event of the copy in flight or None]


def post_persist_abort_read(device):
    """Enqueue an asynchronous read of the abort latch behind everything the current stream holds (train.TrainStep: at the end of a step).  The
    NEXT step looks at the host copy with poll_persist_abort -- no synchronisation: a blocking read at the start of Engine.forward made the host
    wait for the ConvStack the fused step had already enqueued (48 ms) before it planned the decoder and enqueued the encoder (round 5)."""
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    e = _LATCH_READS.get(idx)
    if e is None:
        e = _LATCH_READS[idx] = [torch.zeros(1, dtype=torch.int32).pin_memory(), None]
    if e[1] is not None:
        # the previous step's read was never consumed (a loop without a host synchronisation per step: the poll at the start of this step came
        # before that copy had completed).  It is a whole step old -- waiting for it costs nothing -- and must not be overwritten unseen: an
        # abort would otherwise never be noticed and every following update would be skipped for a NaN loss.
        e[1].synchronize()
        _consume_latch_read(e, device, False)
    e[0].copy_(abort_latch(device), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    e[1] = ev


def poll_persist_abort(device, raise_error=False):
    """Non-blocking form of check_persist_abort: acts on the latch value read by the last post_persist_abort_read once that copy has completed
    (an abort is then noticed one step later at worst; the step it happened in skipped its update on the device anyway).  Before the first
    posted read it falls back to the blocking check (the stream is idle then)."""
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    e = _LATCH_READS.get(idx)
    if e is None:
        return check_persist_abort(device, raise_error)
    if e[1] is None or not e[1].query():
        return 0                          # (still in flight: it stays pending -- the next poll or the next post consumes it)
    return _consume_latch_read(e, device, raise_error)


def _consume_latch_read(e, device, raise_error):
    e[1] = None
    bits = int(e[0][0])
    if not bits:
        return 0
    return _persist_abort_seen(bits, abort_latch(device), raise_error)


def check_persist_abort(device, raise_error=False):
    """Call where the host has just synchronised with the device anyway (a 4-byte read).  If a persistent launch gave up since the last call:
    its outputs were poisoned (NaN loss -> the update was skipped) -- switch the persistent paths off for the rest of the process (the chip is
    evidently shared or partitioned in a way the residency check cannot see) and warn, or raise (greedy decoding: the ids are unusable)."""
    t = abort_latch(device)
    bits = int(t.item())
    if not bits:
        return 0
    return _persist_abort_seen(bits, t, raise_error)


def _persist_abort_seen(bits, t, raise_error):
    global PERSIST_ABORTS
    t.zero_()
    PERSIST_ABORTS += 1
    L = lib()
    L.a2s_debug_set(b"gru_persist", 0)
    L.a2s_debug_set(b"dec_persist", 0)
    os.environ["A2S_DEC_PERSIST"] = "0"
    os.environ["A2S_GRU_PERSIST"] = "0"
    msg = (f"a persistent kernel gave up a bounded wait (latch bits {bits:#x}: 1/2 encoder fwd/bwd, 4/8 note decoder fwd/bwd); its outputs were "
           "poisoned with NaN and the persistent paths are switched off for the rest of this process (launch-per-step kernels from now on)")
    if raise_error:
        raise A2SError(msg)
    import warnings
    warnings.warn(msg, RuntimeWarning)
    return bits


def _p(t):
    """device pointer of a tensor (None -> NULL); tensors must be CUDA(HIP) and of the dtype the C side expects."""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, int):
        return C.c_void_p(t)
    if not t.is_cuda:
        raise A2SError("liba2s_hip operates on device memory only: got a CPU tensor (no CPU fallback exists)")
    return C.c_void_p(t.data_ptr())


def attn_workspace(B, T, H, device, groups=1):
    """Scratch for the split-T attention kernels (None when the one-workgroup-per-clip kernels are used); groups: fused bars per call."""
    if H != 256:
        return None
    # zero-initialised: the head of the workspace holds the arrival counters of the fused combine (left at zero by every launch)
    return torch.zeros(lib().a2s_attn_workspace_floats_fused(B, T, H, groups), dtype=torch.float32, device=device)


def conv_workspace(cin, device):
    n = lib().a2s_conv3x3_workspace_floats(cin)
    return torch.empty(n, dtype=torch.float32, device=device) if n else None


def gemm_workspace(rows, device):
    """Split-K scratch for the per-step skinny GEMMs of the decoder loops (16 slabs of rows x 2048 floats)."""
    return torch.empty(16 * max(rows, 1) * 2048, dtype=torch.float32, device=device)


def gru_workspace(rows, H, device):
    """Workspace of one direction of an encoder GRU layer (a2s_gru_seq_fwd / a2s_gru_seq_bwd): gemm_workspace(rows), and at least what the library
    says the recurrences need at that batch (a2s_gru_workspace_bytes: the transposed W_hh, the step kernels' scratch, the persistent launches'
    granule buffers), so that the backward of a few clips takes the path the forward takes."""
    floats = (lib().a2s_gru_workspace_bytes(max(rows, 1), H) + 3) // 4
    return torch.empty(max(16 * max(rows, 1) * 2048, floats), dtype=torch.float32, device=device)


def step_workspace(H, E, device):
    """Scratch of the fused few-row decoder step kernels (csrc/a2s_step.hip): flags, ticket counters (must start at zero), logits,
    transposed weight copies."""
    return torch.zeros(lib().a2s_note_step_workspace_floats(H, E), dtype=torch.float32, device=device)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def grammar_argmax_rows(x, table, row_state, y=None, V=None):
    """a2s_grammar_argmax_rows: rows of logits x (R, >= V) float32, table (n_states, V) int8 (kern_grammar.KernGrammar.device_table),
    row_state (R,) int32 updated in place -> the emitted ids (R,) int32; y (R, >= V) receives the unconstrained log_softmax when given."""
    V = table.shape[1] if V is None else V
    R = x.shape[0]
    if table.dtype != torch.int8 or row_state.dtype != torch.int32 or x.dtype != torch.float32 or not table.is_contiguous():
        raise A2SError("grammar_argmax_rows: expects float32 logits, a contiguous int8 table and int32 row states")
    choice = torch.empty(R, dtype=torch.int32, device=x.device)
    check(lib().a2s_grammar_argmax_rows(stream(), _p(x), x.stride(0), _p(y), y.stride(0) if y is not None else 0, _p(table), table.shape[0], _p(row_state), _p(choice),
                                        R, V), "a2s_grammar_argmax_rows")
    return choice


def grammar_launches():
    """Grammar step epilogues the library has launched in this process (a2s_grammar_launches)."""
    return int(lib().a2s_grammar_launches())


def metre_ref(metre, row_metre):
    """The metre reference of a kern_grammar.KernMetre and the rows' metre states row_metre (R, 16) int32 on the device (updated in place), as the
    entry points take it: [dur_ticks, cls, fillable, n_fillable, row_metre]."""
    if row_metre.dtype != torch.int32 or row_metre.dim() != 2 or row_metre.shape[1] != 16 or not row_metre.is_contiguous():
        raise A2SError("metre_ref: expects the metre states as a contiguous (R, 16) int32 tensor")
    tb = metre.device_tables(row_metre.device)           # (kept alive by the KernMetre)
    return [_p(tb["dur_ticks"]), _p(tb["cls"]), _p(tb["fillable"]), tb["fillable"].numel(), _p(row_metre)]


def metre_rows(metre, ts_ids):
    """Fresh metre states (R, 16) int32 for rows whose bars have the time-signature ids ts_ids (R,) on the device; an id outside the list of
    time signatures gives L = 0, an unmetred row.  Nothing is read back."""
    ticks = metre.device_tables(ts_ids.device)["bar_ticks"]
    ids = ts_ids.long()
    rows = torch.zeros((ids.shape[0], 16), dtype=torch.int32, device=ts_ids.device)
    rows[:, 0] = torch.where((ids >= 0) & (ids < ticks.numel()), ticks[ids.clamp(0, ticks.numel() - 1)], torch.zeros_like(ticks[:1]))
    rows[:, 2] = 1
    return rows


def metre_argmax_rows(x, table, row_state, metre, row_metre, y=None, V=None):
    """a2s_metre_argmax_rows: grammar_argmax_rows under the metre of kern_grammar.KernMetre `metre`; row_metre (R, 16) int32 is updated in place."""
    V = table.shape[1] if V is None else V
    R = x.shape[0]
    if table.dtype != torch.int8 or row_state.dtype != torch.int32 or x.dtype != torch.float32 or not table.is_contiguous() or row_metre.shape[0] != R:
        raise A2SError("metre_argmax_rows: expects float32 logits, a contiguous int8 table, int32 row states and one metre state per row")
    choice = torch.empty(R, dtype=torch.int32, device=x.device)
    check(lib().a2s_metre_argmax_rows(stream(), _p(x), x.stride(0), _p(y), y.stride(0) if y is not None else 0, _p(table), table.shape[0], _p(row_state),
                                      *metre_ref(metre, row_metre), _p(choice), R, V), "a2s_metre_argmax_rows")
    return choice


def metre_launches():
    """Metre step epilogues the library has launched in this process (a2s_metre_launches)."""
    return int(lib().a2s_metre_launches())


def beam_buffers(B, K, max_steps, V, device, pad_id, table=None, start=0, alpha=0.0):
    """The buffers of one beam-search call (a2s_beam_args) over B clips with K slots: -> (BeamArgs, dict of the tensors it points to).  Scores,
    finished flags and counters are those of the start: slot 0 alive at 0, the others dead; a2s_note_decoder_fwd_beam sets them again itself."""
    R = K * B
    t = dict(row_state=torch.full((R,), start, dtype=torch.int32, device=device),
             score=torch.full((R,), float("-inf"), dtype=torch.float32, device=device),
             finished=torch.ones(R, dtype=torch.int32, device=device),
             done_count=torch.zeros(max_steps + 1, dtype=torch.int32, device=device),
             token_hist=torch.full((max_steps, R), pad_id, dtype=torch.int32, device=device),
             parent_hist=torch.zeros((max_steps, R), dtype=torch.int32, device=device),
             score_hist=torch.zeros((max_steps, R), dtype=torch.float32, device=device),
             probs_scratch=torch.zeros((R, max_steps, V), dtype=torch.float32, device=device),
             ids_out=torch.full((B, max_steps), pad_id, dtype=torch.int32, device=device),
             lengths_out=torch.full((B,), max_steps, dtype=torch.long, device=device),
             score_out=torch.zeros(B, dtype=torch.float32, device=device))
    t["score"][:B] = 0
    t["finished"][:B] = 0
    t["done_count"][0] = (K - 1) * B
    g = BeamArgs()
    g.K, g.alpha, g.pad_id = K, float(alpha), pad_id
    if table is not None:
        if table.dtype != torch.int8 or not table.is_contiguous() or table.shape[1] != V:
            raise A2SError("beam_buffers: expects a contiguous int8 table of (n_states, V)")
        g.next_state, g.n_states = table.data_ptr(), table.shape[0]
        t["table"] = table
    else:
        g.next_state, g.n_states = None, 0
    for name in ("row_state", "score", "finished", "done_count", "token_hist", "parent_hist", "score_hist", "probs_scratch", "ids_out", "lengths_out", "score_out"):
        setattr(g, name, t[name].data_ptr())
    return g, t


def beam_step(g, logits, emb, xnext, h, q, n_done, steps_exec, B, t, max_steps, eos_id, V=None):
    """a2s_beam_step: one beam step epilogue over logits (K * B, >= V); h (K * B, cols) and q (or None) are re-parented in place."""
    V = logits.shape[1] if V is None else V
    check(lib().a2s_beam_step(stream(), C.byref(g), _p(logits), logits.stride(0), _p(emb), _p(xnext), xnext.stride(0), _p(h), h.shape[1], _p(q),
                              q.shape[1] if q is not None else 0, _p(n_done), _p(steps_exec), B, V, emb.shape[1], t, max_steps, eos_id), "a2s_beam_step")


def beam_backtrack(g, probs, steps_exec, B, V, max_steps, eos_id):
    """a2s_beam_backtrack: the pick and the walk back; probs (B, max_steps, V) receives the winning lineage's log-probabilities."""
    check(lib().a2s_beam_backtrack(stream(), C.byref(g), _p(probs), probs.stride(0), _p(steps_exec), B, V, max_steps, eos_id), "a2s_beam_backtrack")


def beam_launches():
    """Beam step epilogues the library has launched in this process (a2s_beam_launches)."""
    return int(lib().a2s_beam_launches())


def attn_align_rows(attw, peak, weight, centroid, T=None, R=None):
    """a2s_attn_align_rows: rows of attention weights attw (R, >= T) float32 -> per row the peak frame (int32), its weight and the centroid
    sum_t t * attw[t] (float32), written to element 0 of row r of peak / weight / centroid (1-D of R elements, or one column of an (R, steps) array:
    the stride of dimension 0 is the output stride the three must share)."""
    R = attw.shape[0] if R is None else R
    T = attw.shape[1] if T is None else T
    if attw.dtype != torch.float32 or peak.dtype != torch.int32 or weight.dtype != torch.float32 or centroid.dtype != torch.float32:
        raise A2SError("attn_align_rows: expects float32 weights, an int32 peak and float32 weight / centroid outputs")
    stride = peak.stride(0) if peak.dim() else 1
    if any((o.stride(0) if o.dim() else 1) != stride or (o.shape[0] if o.dim() else 1) < R for o in (peak, weight, centroid)):
        raise A2SError("attn_align_rows: the three outputs need R rows and one common row stride")
    check(lib().a2s_attn_align_rows(stream(), _p(attw), attw.stride(0) if attw.dim() > 1 else T, R, T, _p(peak), _p(weight), _p(centroid), stride),
          "a2s_attn_align_rows")


def align_launches():
    """attn_align_rows launches of this process (a2s_align_launches)."""
    return int(lib().a2s_align_launches())


def render_notes(programs, n_samples, wave=None):
    """a2s_render_notes: programs (B, 1 + E, 8) int32 on the device (scoregen.pack_program) -> the (B, n_samples) float32 waveforms (written into `wave`,
    a 2-D float32 tensor of at least n_samples columns with unit column stride, when given)."""
    if programs.dim() != 3 or programs.shape[2] != 8 or programs.dtype != torch.int32 or not programs.is_contiguous():
        raise A2SError("render_notes: expects contiguous int32 programs of shape (B, 1 + E, 8)")
    B = programs.shape[0]
    if wave is None:
        wave = torch.empty((B, n_samples), dtype=torch.float32, device=programs.device)
    if wave.dim() != 2 or wave.dtype != torch.float32 or wave.shape[0] < B or wave.shape[1] < n_samples or wave.stride(1) != 1 or wave.device != programs.device:
        raise A2SError("render_notes: the output needs B rows of at least n_samples float32 with unit stride on the programs' device")
    if B == 0:
        return wave                           # (an empty tensor has no data pointer to pass: nothing to launch, as a2s_render_notes with B = 0)
    check(lib().a2s_render_notes(stream(), _p(programs), programs.shape[1], int(n_samples), _p(wave), wave.stride(0), B), "a2s_render_notes")
    return wave


def render_launches():
    """Synthesiser launches of this process (a2s_render_launches)."""
    return int(lib().a2s_render_launches())


def _need(cond, fn, arg, what):
    if not cond:
        raise A2SError(f"{fn}: `{arg}` {what}")


def _features(fn, x):
    """`x` as the augmentation kernels take the features, a contiguous float32 tensor (B, ..., rows, F) on the device -> (B, rows, F); rows = 0 for an
    empty one."""
    _need(torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() >= 3, fn, "x", "must be a float32 tensor (B, ..., rows, F)")
    _need(x.is_contiguous(), fn, "x", "must be contiguous")
    _need(x.is_cuda, fn, "x", "must be on the device")
    B, F = x.shape[0], x.shape[-1]
    return B, (x.numel() // (B * F) if x.numel() else 0), F


def _per_clip(fn, name, t, dtype, x, *trailing):
    """`t` holds something per clip of the features x: a contiguous `dtype` tensor (B, *trailing) on x's device."""
    shape = (x.shape[0],) + trailing
    _need(torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(), fn, name,
          f"must be a contiguous {dtype} tensor " + (f"of shape {shape}" if trailing else f"with one element per clip ({shape[0]})"))
    _need(t.device == x.device, fn, name, "must be on x's device")


def _counters(fn, counters, x):
    _need(torch.is_tensor(counters) and counters.dtype == torch.int32 and counters.numel() == 3 and counters.is_contiguous(), fn, "counters",
          "must be a contiguous int32 tensor of 3 elements")
    _need(counters.device == x.device, fn, "counters", "must be on x's device")


def _like(fn, x, y):
    """`y`, the output of x's shape (a fresh tensor when None): contiguous float32 on x's device."""
    if y is None:
        y = torch.empty_like(x)
    _need(torch.is_tensor(y) and y.dtype == torch.float32 and y.shape == x.shape and y.is_contiguous(), fn, "y", "must be a contiguous float32 tensor of x's shape")
    _need(y.device == x.device, fn, "y", "must be on x's device")
    return y


def transpose_targets(new_key, interval, token_map, semitones, detune, key, upper, lower, bins_per_semitone, eff_bins, counters):
    """a2s_transpose_targets: the tables of kern_transpose.tables() on the device (int32), the draws semitones (B,) int32 and detune (B,) float32, the
    batch's key (B, bars), upper (B, bars, U) and lower (B, bars, L) int64, rewritten IN PLACE where the clip is representable; eff_bins (B,) float32
    receives the feature shift of every clip, counters (3,) int32 grow by [clips, transposed, not representable]."""
    fn = "transpose_targets"
    for name, t, dtype in (("new_key", new_key, torch.int32), ("interval", interval, torch.int32), ("token_map", token_map, torch.int32),
                           ("semitones", semitones, torch.int32), ("detune", detune, torch.float32), ("key", key, torch.int64), ("upper", upper, torch.int64),
                           ("lower", lower, torch.int64), ("eff_bins", eff_bins, torch.float32), ("counters", counters, torch.int32)):
        _need(torch.is_tensor(t) and t.dtype == dtype, fn, name, f"must be a {dtype} tensor")
        _need(t.is_contiguous(), fn, name, "must be contiguous")
    _need(token_map.dim() == 2, fn, "token_map", "must be (rows, V)")
    _need(tuple(new_key.shape) == (13, 14), fn, "new_key", "must be (13, 14)")
    _need(tuple(interval.shape) == (13, 14), fn, "interval", "must be (13, 14)")
    _need(key.dim() == 2, fn, "key", "must be (B, bars)")
    B, bars = key.shape
    _need(upper.dim() == 3 and tuple(upper.shape[:2]) == (B, bars), fn, "upper", f"must be ({B}, {bars}, U) as `key` says")
    _need(lower.dim() == 3 and tuple(lower.shape[:2]) == (B, bars), fn, "lower", f"must be ({B}, {bars}, L) as `key` says")
    for name, t in (("semitones", semitones), ("detune", detune), ("eff_bins", eff_bins)):
        _need(tuple(t.shape) == (B,), fn, name, f"must have one element per clip ({B})")
    _need(counters.numel() == 3, fn, "counters", "must have 3 elements")
    if B == 0:
        return
    check(lib().a2s_transpose_targets(stream(), _p(new_key), _p(interval), _p(token_map), token_map.shape[0], token_map.shape[1], _p(semitones), _p(detune),
                                      _p(key), _p(upper), _p(lower), bars, upper.shape[2], lower.shape[2], int(bins_per_semitone), _p(eff_bins), _p(counters), B),
          "a2s_transpose_targets")


def shift_bins(x, eff_bins, y=None):
    """a2s_shift_bins: x (B, ..., rows, F) float32, contiguous -> y of the same shape (a fresh tensor when not given), every row of clip b shifted
    by eff_bins[b] bins (float32 on the device; fractional shifts interpolate linearly, what falls outside [0, F) is zero)."""
    fn = "shift_bins"
    B, rows, F = _features(fn, x)
    _per_clip(fn, "eff_bins", eff_bins, torch.float32, x)
    y = _like(fn, x, y)
    if x.numel() == 0:
        return y
    check(lib().a2s_shift_bins(stream(), _p(x), _p(y), _p(eff_bins), B, rows, F), "a2s_shift_bins")
    return y


def augment_launches():
    """Launches of the two augmentation kernels in this process (a2s_augment_launches)."""
    return int(lib().a2s_augment_launches())


def tempo_plan(x, u, R, min_frames, content, step, counters):
    """a2s_tempo_plan: x (B, ..., rows, F) float32, contiguous; u (B,) float32 in [0, 1), the host's draws; R in [0, 0.25] the largest relative change
    of the durations, min_frames >= 1 the least content a stretched clip keeps.  content (B,) int32 receives 1 + the last non-zero row of every clip,
    step (B,) int32 the Q16 source advance per output row that a2s_stretch_frames reads; counters (3,) int32 grow by [clips, stretched, kept]."""
    fn = "tempo_plan"
    B, rows, F = _features(fn, x)
    for name, t, dtype in (("u", u, torch.float32), ("content", content, torch.int32), ("step", step, torch.int32)):
        _per_clip(fn, name, t, dtype, x)
    _counters(fn, counters, x)
    try:
        Rf, mf = float(R), int(min_frames)
    except (TypeError, ValueError):
        raise A2SError(f"{fn}: `R` and `min_frames` must be numbers (got {R!r}, {min_frames!r})") from None
    _need(0.0 <= Rf <= 0.25, fn, "R", f"must be in 0 .. 0.25 (got {R!r})")
    _need(mf >= 1 and mf == min_frames, fn, "min_frames", f"must be a whole number >= 1 (got {min_frames!r})")
    if x.numel() == 0:
        return
    _need(rows <= 16384, fn, "x", f"has {rows} rows per clip, more than 16384")
    check(lib().a2s_tempo_plan(stream(), _p(x), B, rows, F, _p(u), Rf, mf, _p(content), _p(step), _p(counters)), "a2s_tempo_plan")


def stretch_frames(x, step, y=None):
    """a2s_stretch_frames: x (B, ..., rows, F) float32, contiguous -> y of the same shape (a fresh tensor when not given), the rows of clip b resampled
    with the Q16 source advance step[b] per output row (int32 on the device; 65536: a copy; below: linear interpolation, the clip gets longer; above: a
    widened tent, it gets shorter; outside 52429 .. 87381: zeros)."""
    fn = "stretch_frames"
    B, rows, F = _features(fn, x)
    _per_clip(fn, "step", step, torch.int32, x)
    y = _like(fn, x, y)
    if x.numel() == 0:
        return y
    _need(rows <= 16384, fn, "x", f"has {rows} rows per clip, more than 16384")
    check(lib().a2s_stretch_frames(stream(), _p(x), _p(y), _p(step), B, rows, F), "a2s_stretch_frames")
    return y


def tempo_launches():
    """Launches of the two tempo kernels in this process (a2s_tempo_launches; a2s_augment_launches does not count them)."""
    return int(lib().a2s_tempo_launches())


def _specaug_args(fn, x, table, content, plan, stats):
    """The checks specaug_plan and specaug_apply share -> (B, rows, F)."""
    B, rows, F = _features(fn, x)
    _per_clip(fn, "table", table, torch.float32, x, 2, F)
    _per_clip(fn, "content", content, torch.int32, x)
    _per_clip(fn, "plan", plan, torch.int32, x, 16)
    _per_clip(fn, "stats", stats, torch.float32, x, 2)
    return B, rows, F


def specaug_plan(x, table, draws, Wt, Wf, m, content, plan, stats, counters):
    """a2s_specaug_plan: x (B, ..., rows, F) float32, contiguous; table (B, 2, F) float32, per clip the power gains G_k > 0 and the noise powers
    v_k >= 0; draws (B, 16) int32, the host's 32-bit draws (the bits of its uint32 words), four per mask; Wt, Wf >= 0 the largest mask widths in rows
    and bins, m in 0 .. 4 the masks of each kind.  content (B,) int32 receives 1 + the last non-zero row of every clip, plan (B, 16) int32
    4 x [t0, w] then 4 x [k0, wk], stats (B, 2) float32 [x_min, M]; counters (3,) int32 grow by [clips, time-masked, frequency-masked]."""
    fn = "specaug_plan"
    B, rows, F = _specaug_args(fn, x, table, content, plan, stats)
    _per_clip(fn, "draws", draws, torch.int32, x, 16)          # (the bits of the 32-bit draws)
    _counters(fn, counters, x)
    try:
        wt, wf, mi = int(Wt), int(Wf), int(m)
    except (TypeError, ValueError):
        raise A2SError(f"{fn}: `Wt`, `Wf` and `m` must be whole numbers (got {Wt!r}, {Wf!r}, {m!r})") from None
    _need(wt >= 0 and wt == Wt, fn, "Wt", f"must be a whole number >= 0 (got {Wt!r})")
    _need(wf >= 0 and wf == Wf, fn, "Wf", f"must be a whole number >= 0 (got {Wf!r})")
    _need(0 <= mi <= 4 and mi == m, fn, "m", f"must be a whole number in 0 .. 4 (got {m!r})")
    if x.numel() == 0:
        return
    check(lib().a2s_specaug_plan(stream(), _p(x), B, rows, F, _p(table), _p(draws), wt, wf, mi, _p(content), _p(plan), _p(stats), _p(counters)),
          "a2s_specaug_plan")


def specaug_apply(x, table, content, plan, stats, y=None):
    """a2s_specaug_apply: x (B, ..., rows, F) float32, contiguous -> y of the same shape (a fresh tensor when not given): every clip coloured by its
    table (B, 2, F), re-normalised to its new peak and masked, with content, plan and stats as specaug_plan left them."""
    fn = "specaug_apply"
    B, rows, F = _specaug_args(fn, x, table, content, plan, stats)
    y = _like(fn, x, y)
    _need(y.data_ptr() != x.data_ptr() or x.numel() == 0, fn, "y", "must not be x: the kernel works out of place")
    if x.numel() == 0:
        return y
    check(lib().a2s_specaug_apply(stream(), _p(x), _p(y), _p(table), _p(content), _p(plan), _p(stats), B, rows, F), "a2s_specaug_apply")
    return y


def specaug_launches():
    """Launches of the two spectrogram-augmentation kernels in this process (a2s_specaug_launches; the other augmenters' counters do not count them)."""
    return int(lib().a2s_specaug_launches())


def _room_table(fn, params, seeds=None):
    _need(torch.is_tensor(params) and params.dtype == torch.int32 and params.dim() == 2 and params.shape[1] == 4 and params.is_contiguous() and params.is_cuda,
          fn, "params", "must be a contiguous (B, 4) int32 tensor on the device: [pre, L, wet f32 bits, decay f32 bits] per clip")
    if seeds is not None:
        _need(torch.is_tensor(seeds) and seeds.dtype == torch.int32 and tuple(seeds.shape) == (params.shape[0],) and seeds.is_contiguous()
              and seeds.device == params.device, fn, "seeds", f"must be a contiguous int32 tensor (the 32 bits of every clip's seed) of {params.shape[0]} elements on the table's device")
    return params.shape[0]


def _rows(fn, name, t, B, n, device):
    _need(torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] >= B and t.shape[1] >= n and t.device == device
          and (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= n), fn, name,
          f"must be a float32 tensor of at least {B} rows of at least {n} elements with unit stride on the table's device")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), n)


def room_ir(seeds, params, L_max, ir=None):
    """a2s_room_ir: seeds (B,) int32 (the bits of the clips' 32-bit room seeds) and params (B, 4) int32 on the device -> ir (B, L_max) float32, the
    impulse response of every clip (written into `ir`, a 2-D float32 tensor of at least L_max columns with unit column stride, when given)."""
    fn = "room_ir"
    B = _room_table(fn, params, seeds)
    L_max = int(L_max)
    _need(L_max >= 1, fn, "L_max", f"must be >= 1 (got {L_max})")
    if ir is None:
        ir = torch.empty((B, L_max), dtype=torch.float32, device=params.device)
    stride = _rows(fn, "ir", ir, B, L_max, params.device)
    if B == 0:
        return ir
    check(lib().a2s_room_ir(stream(), _p(seeds), _p(params), B, _p(ir), stride, L_max), "a2s_room_ir")
    return ir


def fir_rows(x, ir, params, L_max, y=None, n_samples=None):
    """a2s_fir_rows: x (B, N) float32 waveforms, ir (B, >= L_max) float32 and params (B, 4) int32 on the device -> y (B, n_samples) float32 (a fresh
    tensor when not given), y[b][n] = sum_{k <= min(L[b] - 1, n)} ir[b][k] x[b][n - k] with L[b] = clamp(params[b][1], 1, L_max).  Out of place."""
    fn = "fir_rows"
    B = _room_table(fn, params)
    L_max = int(L_max)
    _need(L_max >= 1, fn, "L_max", f"must be >= 1 (got {L_max})")
    _need(torch.is_tensor(x) and x.dim() == 2, fn, "x", "must be a 2-D float32 tensor")
    n = x.shape[1] if n_samples is None else int(n_samples)
    _need(n >= 1 or B == 0, fn, "n_samples", f"must be >= 1 (got {n})")
    xs = _rows(fn, "x", x, B, n, params.device)
    irs = _rows(fn, "ir", ir, B, L_max, params.device)
    if y is None:
        y = torch.empty((B, n), dtype=torch.float32, device=params.device)
    ys = _rows(fn, "y", y, B, n, params.device)
    if B == 0:
        return y
    _need(x.data_ptr() != y.data_ptr(), fn, "y", "must not be x (the convolution works out of place)")
    check(lib().a2s_fir_rows(stream(), _p(x), xs, _p(ir), irs, _p(params), _p(y), ys, B, n, L_max), "a2s_fir_rows")
    return y


def fir_tile_samples():
    """Samples per workgroup of a2s_fir_rows."""
    return int(lib().a2s_fir_tile_samples())


def fir_tap_chunk():
    """Taps per staged window of a2s_fir_rows."""
    return int(lib().a2s_fir_tap_chunk())


def room_launches():
    """Launches of the two room kernels in this process (a2s_room_launches)."""
    return int(lib().a2s_room_launches())


def resample_rows(x, n_in, table, M, Hh, channels=1, y=None, n_out_max=None, n_in_max=None):
    """a2s_resample_rows: x (B, >= n_in_max * channels) float32 rows of interleaved frames, n_in (B,) int32 frames per clip and table (L, K) float32 on the
    device -> y (B, n_out_max) float32 (a fresh tensor when not given): the mono mix of every clip resampled by L / M, y[b][n] = sum_i table[p][i] *
    mono_b[m0 + Hh - i] with p = n M mod L, m0 = n M div L, zero at and behind ceil(n_in[b] L / M).  n_in_max (default: the frames a row of x holds)
    bounds n_in on the device, n_out_max defaults to ceil(n_in_max L / M).  Out of place."""
    fn = "resample_rows"
    _need(torch.is_tensor(table) and table.dtype == torch.float32 and table.dim() == 2 and table.is_contiguous() and table.is_cuda and table.numel() > 0, fn,
          "table", "must be a contiguous (L, K) float32 tensor on the device")
    L, K = table.shape
    try:
        M, Hh, C = int(M), int(Hh), int(channels)
    except (TypeError, ValueError):
        raise A2SError(f"{fn}: `M`, `Hh` and `channels` must be whole numbers (got {M!r}, {Hh!r}, {channels!r})") from None
    _need(1 <= C <= 8, fn, "channels", f"must be in 1 .. 8 (got {C})")
    _need(1 <= L <= 4096, fn, "table", f"must have 1 .. 4096 rows (got {L})")
    _need(1 <= K <= 8192, fn, "table", f"must have 1 .. 8192 columns (got {K})")
    _need(1 <= M <= 4096, fn, "M", f"must be in 1 .. 4096 (got {M})")
    _need(0 <= Hh < K, fn, "Hh", f"must be in 0 .. K - 1 = {K - 1} (got {Hh})")
    _need(torch.is_tensor(n_in) and n_in.dtype == torch.int32 and n_in.dim() == 1 and n_in.is_contiguous() and n_in.device == table.device, fn, "n_in",
          "must be a contiguous int32 tensor of one element per clip on the table's device")
    B = n_in.shape[0]
    _need(torch.is_tensor(x) and x.dim() == 2, fn, "x", "must be a 2-D float32 tensor of interleaved frames")
    nim = x.shape[1] // C if n_in_max is None else int(n_in_max)
    _need(nim >= 0, fn, "n_in_max", f"must be >= 0 (got {nim})")
    nom = -(-nim * L // M) if n_out_max is None else int(n_out_max)
    _need(nom >= 1 or B == 0, fn, "n_out_max", f"must be >= 1 (got {nom})")
    xs = _rows(fn, "x", x, B, nim * C, table.device)
    if y is None:
        y = torch.empty((B, max(nom, 0)), dtype=torch.float32, device=table.device)
    ys = _rows(fn, "y", y, B, nom, table.device)
    if B == 0:
        return y
    _need(x.data_ptr() != y.data_ptr(), fn, "y", "must not be x (the resampler works out of place)")
    check(lib().a2s_resample_rows(stream(), _p(x), xs, _p(n_in), nim, C, _p(table), L, M, K, Hh, _p(y), ys, nom, B), "a2s_resample_rows")
    return y


def resample_tile_samples():
    """Outputs per workgroup of a2s_resample_rows."""
    return int(lib().a2s_resample_tile_samples())


def resample_launches():
    """Launches of the resampler in this process (a2s_resample_launches)."""
    return int(lib().a2s_resample_launches())


def _whole(fn, **values):
    """The named arguments as Python ints; a value that is no whole number is an error that names it."""
    out = []
    for name, v in values.items():
        try:
            i = int(v)
        except (TypeError, ValueError):
            i = None
        _need(i is not None and i == v, fn, name, f"must be a whole number (got {v!r})")
        out.append(i)
    return out


def _int_rows(fn, name, t, shape, device):
    _need(torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == device, fn, name,
          f"must be a contiguous int32 tensor of shape {tuple(shape)} on the device of the first argument")


def onset_strength(x, n_rows, lag=1, f_split=180, env_full=None, env_low=None):
    """a2s_onset_strength: x (B, rows, F) or (B, 1, rows, F) float32 on the device, unit stride along F (the rows and the clips may be strided), n_rows
    (B,) int32 -> (env_full, env_low), (B, rows) float32 each (fresh tensors when not given; given ones are 2-D with unit column stride):
    env_full[b][t] = sum_f max(0, x[b][t][f] - x[b][t - lag][f]) for lag <= t < n_rows[b], 0 elsewhere; env_low the same over f < f_split."""
    fn = "onset_strength"
    _need(torch.is_tensor(x) and x.dtype == torch.float32 and x.is_cuda and (x.dim() == 3 or (x.dim() == 4 and x.shape[1] == 1)), fn, "x",
          "must be a float32 tensor (B, rows, F) or (B, 1, rows, F) on the device")
    if x.dim() == 4:
        x = x[:, 0]
    B, rows, F = x.shape
    lag, f_split = _whole(fn, lag=lag, f_split=f_split)
    _need(lag >= 1, fn, "lag", f"must be >= 1 (got {lag})")
    _need(0 <= f_split <= F, fn, "f_split", f"must be in 0 .. F = {F} (got {f_split})")
    _int_rows(fn, "n_rows", n_rows, (B,), x.device)
    outs = []
    for name, t in (("env_full", env_full), ("env_low", env_low)):
        if t is None:
            t = torch.empty((B, rows), dtype=torch.float32, device=x.device)
        outs.append(t)
    if B == 0 or rows == 0 or F == 0:
        _need(B == 0 or F > 0 or rows == 0, fn, "x", "has rows but no columns")
        return tuple(outs)
    _need(x.stride(2) == 1 or F == 1, fn, "x", "must have unit stride along F")
    xr = x.stride(1) if rows > 1 else max(x.stride(1), F)
    xb = x.stride(0) if B > 1 else max(x.stride(0), (rows - 1) * xr + F)
    _need(xr >= F and xb >= (rows - 1) * xr + F, fn, "x", f"has overlapping rows or clips (strides {tuple(x.stride())})")
    es = _rows(fn, "env_full", outs[0], B, rows, x.device)
    _need(_rows(fn, "env_low", outs[1], B, rows, x.device) == es, fn, "env_low", "must have env_full's row stride")
    _need(lag * (-(-F // 4) * 4) <= 12288, fn, "lag", f"times F = {F} exceeds the 12288 floats a workgroup keeps (got {lag})")
    check(lib().a2s_onset_strength(stream(), _p(x), xb, xr, _p(n_rows), B, rows, F, lag, f_split, _p(outs[0]), _p(outs[1]), es), "a2s_onset_strength")
    return tuple(outs)


def tempogram(env, n, win=800, hop_b=100, lag_min=20, lag_max=200, J=None, out=None):
    """a2s_tempogram: env (R, stride) float32 on the device (unit column stride), n (R,) int32 frames per recording -> out (R, J, lag_max - lag_min + 1)
    float32, contiguous (a fresh tensor when not given): the normalised autocorrelation of the mean-free window of `win` frames centred at frame
    j * hop_b, at the lags lag_min .. lag_max.  J defaults to max(1, ceil(stride / hop_b))."""
    fn = "tempogram"
    _need(torch.is_tensor(env) and env.dtype == torch.float32 and env.dim() == 2 and env.is_cuda, fn, "env", "must be a 2-D float32 tensor on the device")
    R, width = env.shape
    win, hop_b, lag_min, lag_max = _whole(fn, win=win, hop_b=hop_b, lag_min=lag_min, lag_max=lag_max)
    _need(1 <= win <= 8192, fn, "win", f"must be in 1 .. 8192 (got {win})")
    _need(hop_b >= 1, fn, "hop_b", f"must be >= 1 (got {hop_b})")
    _need(0 <= lag_min <= lag_max and lag_max - lag_min < 4096, fn, "lag_min", f"and lag_max must satisfy 0 <= lag_min <= lag_max, at most 4096 lags (got {lag_min}, {lag_max})")
    J = max(1, -(-width // hop_b)) if J is None else _whole(fn, J=J)[0]
    _need(J >= 1, fn, "J", f"must be >= 1 (got {J})")
    _int_rows(fn, "n", n, (R,), env.device)
    nl = lag_max - lag_min + 1
    if out is None:
        out = torch.empty((R, J, nl), dtype=torch.float32, device=env.device)
    _need(torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (R, J, nl) and out.is_contiguous() and out.device == env.device, fn, "out",
          f"must be a contiguous float32 tensor of shape {(R, J, nl)} on env's device")
    if R == 0:
        return out
    _need(width >= 1, fn, "env", "has no columns")
    stride = _rows(fn, "env", env, R, width, env.device)
    check(lib().a2s_tempogram(stream(), _p(env), stride, _p(n), R, J, win, hop_b, lag_min, lag_max, _p(out)), "a2s_tempogram")
    return out


def beat_dp(ls, period, pen, n, hop_b=100, lag_min=20, max_beats=None, S=None, back=None, beats=None, count=None):
    """a2s_beat_dp: ls (R, stride) float32 (the envelope over its standard deviation), period (R, J) int32, pen (lag_max - lag_min + 1, 2 lag_max + 1)
    float32 (beats.penalty_table), n (R,) int32, all on the device -> (S (R, stride) float32, back (R, stride) int32, beats (R, max_beats) int32,
    count (R,) int32), fresh tensors where not given (S and back zero-filled, beats filled with -1: the kernel writes [0, n) and the first
    min(count, max_beats) beats only).  count is the true number of beats also where it exceeds max_beats (default stride // ceil(lag_min / 2) + 1,
    which it cannot exceed)."""
    fn = "beat_dp"
    _need(torch.is_tensor(ls) and ls.dtype == torch.float32 and ls.dim() == 2 and ls.is_contiguous() and ls.is_cuda, fn, "ls",
          "must be a contiguous 2-D float32 tensor on the device")
    R, stride = ls.shape
    hop_b, lag_min = _whole(fn, hop_b=hop_b, lag_min=lag_min)
    _need(hop_b >= 1, fn, "hop_b", f"must be >= 1 (got {hop_b})")
    _need(torch.is_tensor(pen) and pen.dtype == torch.float32 and pen.dim() == 2 and pen.is_contiguous() and pen.device == ls.device, fn, "pen",
          "must be a contiguous 2-D float32 tensor on ls's device")
    lag_max = (pen.shape[1] - 1) // 2
    _need(lag_min >= 1 and pen.shape[1] == 2 * lag_max + 1 and pen.shape[0] == lag_max - lag_min + 1 and lag_max <= 4096, fn, "pen",
          f"must have lag_max - lag_min + 1 rows of 2 lag_max + 1 columns, 1 <= lag_min <= lag_max <= 4096 (got {tuple(pen.shape)} for lag_min = {lag_min})")
    _need(torch.is_tensor(period) and period.dim() == 2 and period.shape[1] >= 1, fn, "period", "must be a 2-D int32 tensor (R, J), J >= 1")
    _int_rows(fn, "period", period, (R, period.shape[1]), ls.device)
    _int_rows(fn, "n", n, (R,), ls.device)
    max_beats = stride // ((lag_min + 1) // 2) + 1 if max_beats is None else _whole(fn, max_beats=max_beats)[0]
    _need(max_beats >= 1, fn, "max_beats", f"must be >= 1 (got {max_beats})")
    S = torch.zeros((R, stride), dtype=torch.float32, device=ls.device) if S is None else S
    back = torch.zeros((R, stride), dtype=torch.int32, device=ls.device) if back is None else back
    beats = torch.full((R, max_beats), -1, dtype=torch.int32, device=ls.device) if beats is None else beats
    count = torch.zeros((R,), dtype=torch.int32, device=ls.device) if count is None else count
    _need(torch.is_tensor(S) and S.dtype == torch.float32 and tuple(S.shape) == (R, stride) and S.is_contiguous() and S.device == ls.device, fn, "S",
          f"must be a contiguous float32 tensor of shape {(R, stride)} on ls's device")
    _int_rows(fn, "back", back, (R, stride), ls.device)
    _int_rows(fn, "beats", beats, (R, max_beats), ls.device)
    _int_rows(fn, "count", count, (R,), ls.device)
    if R == 0:
        return S, back, beats, count
    _need(stride >= 1, fn, "ls", "has no columns")
    check(lib().a2s_beat_dp(stream(), _p(ls), stride, _p(period), period.shape[1], hop_b, _p(pen), lag_min, lag_max, _p(n), R, _p(S), _p(back), _p(beats),
                            max_beats, _p(count)), "a2s_beat_dp")
    return S, back, beats, count


def beat_launches():
    """Launches of the three beat-tracking kernels in this process (a2s_beat_launches)."""
    return int(lib().a2s_beat_launches())


def segment_agreement(x, y, seg):
    """a2s_segment_agreement: x, y float32 tensors of one shape (B, T, F) or (B, 1, T, F) on the device, unit stride along F, rows contiguous (row
    stride F; the clips may lie further apart, both tensors with the same clip stride); seg: the HOST table, anything numpy reads as whole numbers of
    shape (S, 3) [clip, f0, f1] or (S, 4) -> (S, 5) float64 on the device: [sum x, sum y, sum x^2, sum y^2, sum x y] over x[clip][f0:f1][:].
    The table is checked here, before it is uploaded: 0 <= clip < B and 0 <= f0 <= f1 <= T (an empty range is allowed and gives zeros)."""
    x, y, (B, T, F), t64, stride = _segment_operands("segment_agreement", x, y, seg)
    S = t64.shape[0]
    out = torch.zeros((S, 5), dtype=torch.float64, device=x.device)
    if S == 0:
        return out
    host = np.zeros((S, 4), dtype=np.int32)
    host[:, :3] = t64[:, :3]
    dev = torch.from_numpy(host).to(x.device)
    check(lib().a2s_segment_agreement(stream(), _p(x), _p(y), stride, B, T, F, _p(dev), S, _p(out)), "a2s_segment_agreement")
    return out


def _feature_pair(fn, x, y):
    """x, y: float32 tensors of one shape (B, T, F) or (B, 1, T, F) on one device -> both as (B, T, F) views."""
    for name, t in (("x", x), ("y", y)):
        _need(torch.is_tensor(t) and t.dtype == torch.float32 and t.is_cuda and (t.dim() == 3 or (t.dim() == 4 and t.shape[1] == 1)), fn, name,
              "must be a float32 tensor (B, T, F) or (B, 1, T, F) on the device")
    if x.dim() == 4:
        x = x[:, 0]
    if y.dim() == 4:
        y = y[:, 0]
    _need(x.shape == y.shape and x.device == y.device, fn, "y", f"must have x's shape and device (got {tuple(y.shape)} for {tuple(x.shape)})")
    return x, y


def _clip_stride(fn, x, y):
    """The clip stride two (B, T, F) views share: unit stride along F, rows contiguous, clips at least T * F apart."""
    B, T, F = x.shape
    strides = []
    for name, t in (("x", x), ("y", y)):
        _need((t.stride(2) == 1 or F == 1) and (t.stride(1) == F or T == 1), fn, name, f"must have contiguous rows (strides {tuple(t.stride())})")
        strides.append(t.stride(0) if B > 1 else T * F)
    _need(strides[0] == strides[1] and strides[0] >= T * F, fn, "y", f"must have x's clip stride, at least T * F (got {strides[1]} and {strides[0]})")
    return strides[0]


def _segment_operands(fn, x, y, seg):
    """The checks a2s_segment_agreement and the DTW entry points share -> (x and y as (B, T, F) views, (B, T, F), the host table as int64 (S, 3 or 4),
    the clip stride -- None where S == 0: an empty table asks nothing of the tensors' cells)."""
    x, y = _feature_pair(fn, x, y)
    B, T, F = x.shape
    _need(not torch.is_tensor(seg) or not seg.is_cuda, fn, "seg", "is the host table (it is checked before it is uploaded)")
    try:
        table = np.asarray(seg.numpy() if torch.is_tensor(seg) else seg)
        whole = table.size == 0 or (np.issubdtype(table.dtype, np.integer) or bool(np.all(table == np.rint(table))))
    except (TypeError, ValueError):
        table, whole = None, False
    _need(whole, fn, "seg", "must hold whole numbers")
    table = table.reshape(0, 4) if table.size == 0 else table
    _need(table.ndim == 2 and table.shape[1] in (3, 4), fn, "seg", f"must be (S, 3) or (S, 4) (got {table.shape})")
    t64 = table.astype(np.int64)
    if t64.shape[0] == 0:
        return x, y, (B, T, F), t64, None
    _need(B >= 1 and T >= 1 and F >= 1, fn, "x", f"has no cells (shape {tuple(x.shape)}) but the table has segments")
    bad = np.nonzero((t64[:, 0] < 0) | (t64[:, 0] >= B) | (t64[:, 1] < 0) | (t64[:, 1] > t64[:, 2]) | (t64[:, 2] > T))[0]
    _need(bad.size == 0, fn, "seg", f"row {int(bad[0]) if bad.size else 0} = {t64[bad[0], :3].tolist() if bad.size else []} is outside 0 <= clip < {B}, 0 <= f0 <= f1 <= {T}")
    return x, y, (B, T, F), t64, _clip_stride(fn, x, y)


DTW_T_MAX = 4096          # the longest clip a2s_dtw_cost / a2s_dtw_path take (csrc/a2s_dtw.hip)


def dtw_geometry(table):
    """(n_max, r_max) that hold every row [clip, f0, f1, r] of the int64 host table: the buffers of a2s_dtw_cost / a2s_dtw_path are sized by them
    (include/a2s.h).  r_max = -1 where the widest block is a full square."""
    n = table[:, 2] - table[:, 1]
    r = table[:, 3]
    banded = (r >= 0) & (2 * r + 1 < n)
    width = np.where(banded, 2 * r + 1, n)
    n_max, need = max(1, int(n.max())), int(width.max())
    return n_max, (-1 if need >= n_max else need // 2)


def dtw_cost(x, y, seg, off=None):
    """a2s_dtw_cost: x, y and the HOST table seg as for segment_agreement, the table (S, 4) [clip, f0, f1, r] (or (S, 3): no band), S >= 1; off None or
    (S,) float32 on the device -> (cost: flat float32 device tensor in the block layout of include/a2s.h, zero where the kernel does not write, the
    table on the device (S, 4) int32, (B, T, n_max, r_max))."""
    fn = "dtw_cost"
    x, y, (B, T, F), t64, stride = _segment_operands(fn, x, y, seg)
    S = t64.shape[0]
    _need(S >= 1, fn, "seg", "must hold at least one segment")
    _need(T <= DTW_T_MAX, fn, "x", f"must have at most {DTW_T_MAX} rows per clip (got {T})")
    host = np.full((S, 4), -1, dtype=np.int64)
    host[:, :t64.shape[1]] = t64
    _need(bool(np.all(np.abs(host[:, 3]) < 2 ** 31)), fn, "seg", "holds a band width that is no int32")
    if off is not None:
        _need(torch.is_tensor(off) and off.dtype == torch.float32 and off.device == x.device and tuple(off.shape) == (S,) and off.is_contiguous(), fn, "off",
              f"must be a contiguous float32 tensor ({S},) on x's device")
    n_max, r_max = dtw_geometry(host)
    dev = torch.from_numpy(host.astype(np.int32)).to(x.device)
    cost = torch.zeros(int(lib().a2s_dtw_cost_bytes(S, n_max, r_max)) // 4, dtype=torch.float32, device=x.device)
    check(lib().a2s_dtw_cost(stream(), _p(x), _p(y), stride, B, T, F, _p(dev), S, None if off is None else _p(off), n_max, r_max, _p(cost), cost.numel() * 4),
          "a2s_dtw_cost")
    return cost, dev, (B, T, n_max, r_max)


def dtw_path(cost, dev, geometry):
    """a2s_dtw_path on what dtw_cost returned (or on any cost buffer of that layout) -> (paths (S, 2 n_max - 1) int32, -1 behind a row's steps; steps
    (S,) int32; totals (S,) float32), on the device."""
    fn = "dtw_path"
    B, T, n_max, r_max = (int(v) for v in geometry)
    _need(torch.is_tensor(dev) and dev.dtype == torch.int32 and dev.is_cuda and dev.dim() == 2 and dev.shape[1] == 4 and dev.is_contiguous(), fn, "dev",
          "must be the contiguous int32 table (S, 4) on the device")
    S = dev.shape[0]
    need = int(lib().a2s_dtw_cost_bytes(S, n_max, r_max)) // 4
    _need(torch.is_tensor(cost) and cost.dtype == torch.float32 and cost.device == dev.device and cost.is_contiguous() and cost.numel() >= need, fn, "cost",
          f"must be a contiguous float32 tensor of at least {need} elements on the table's device")
    ws = torch.zeros(int(lib().a2s_dtw_workspace_bytes(S, n_max, r_max)), dtype=torch.uint8, device=dev.device)
    paths = torch.full((S, 2 * n_max - 1), -1, dtype=torch.int32, device=dev.device)
    steps = torch.zeros((S,), dtype=torch.int32, device=dev.device)
    totals = torch.zeros((S,), dtype=torch.float32, device=dev.device)
    if S == 0:
        return paths, steps, totals
    check(lib().a2s_dtw_path(stream(), _p(dev), S, B, T, n_max, r_max, _p(cost), cost.numel() * 4, _p(ws), ws.numel(), _p(paths), _p(steps), _p(totals)),
          "a2s_dtw_path")
    return paths, steps, totals


def dtw_segments(x, y, seg, off=None):
    """Dynamic time warping of y onto x, segment by segment (a2s_dtw_cost, then a2s_dtw_path): x, y and the HOST table as for
    segment_agreement, the table (S, 4) [clip, f0, f1, r] with the Sakoe-Chiba half-width r (r < 0 or r >= f1 - f0: no band; (S, 3): no band); off None
    or (S,) float32 on the device, subtracted from every difference x - y of the segment -> (paths (S, 2 n_max - 1) int32, entry k of row s =
    (i << 16) | j, ascending from (0, 0) to (n - 1, n - 1), -1 behind the row's steps; steps (S,) int32; totals (S,) float32), on the device."""
    if _segment_operands("dtw_segments", x, y, seg)[3].shape[0] == 0:
        return (torch.zeros((0, 1), dtype=torch.int32, device=x.device), torch.zeros((0,), dtype=torch.int32, device=x.device),
                torch.zeros((0,), dtype=torch.float32, device=x.device))
    cost, dev, geometry = dtw_cost(x, y, seg, off)
    return dtw_path(cost, dev, geometry)


def dtw_launches():
    """Launches of the two DTW kernels in this process (a2s_dtw_launches)."""
    return int(lib().a2s_dtw_launches())


NOTE_ROWS_MAX = 512          # note rows per clip a2s_note_amp_update takes (csrc/a2s_dynamics.hip)


def note_table(rows, first, n_clips, program_rows, device):
    """The HOST note table of the dynamics kernels, checked and uploaded once: rows (S, 8) whole numbers [clip, fx, fy, n, b1,
    b2, b3, prog_row], first (n_clips + 1,) the clips' offsets; program_rows: rows of one render program, header included.  The rows of clip b are
    rows[first[b]:first[b + 1]], at most NOTE_ROWS_MAX, every one with clip == b and 1 <= prog_row < program_rows (the update kernel cannot refuse a
    row: it reads nothing back) -> (rows, first) as contiguous int32 tensors on `device`."""
    fn = "note_table"
    try:
        r, f = np.asarray(rows), np.asarray(first)
        whole = all(t.size == 0 or np.issubdtype(t.dtype, np.integer) or bool(np.all(t == np.rint(t))) for t in (r, f))
    except (TypeError, ValueError):
        r, f, whole = None, None, False
    _need(whole, fn, "rows", "and `first` must hold whole numbers")
    r = r.reshape(0, 8) if r.size == 0 else r
    _need(r.ndim == 2 and r.shape[1] == 8 and bool(np.all(np.abs(r.astype(np.int64)) < 2 ** 31)), fn, "rows", f"must be (S, 8) int32 values (got {r.shape})")
    r, f = r.astype(np.int64), f.astype(np.int64).reshape(-1)
    S = r.shape[0]
    _need(n_clips >= 1 and f.shape == (n_clips + 1,) and f[0] == 0 and f[-1] == S and bool(np.all(np.diff(f) >= 0)), fn, "first",
          f"must hold {n_clips + 1} ascending offsets from 0 to S = {S}")
    _need(bool(np.all(np.diff(f) <= NOTE_ROWS_MAX)), fn, "first", f"gives a clip more than {NOTE_ROWS_MAX} rows")
    _need(bool(np.array_equal(r[:, 0], np.repeat(np.arange(n_clips), np.diff(f)))), fn, "rows", "of one clip must be contiguous, in the order of `first`")
    bad = np.nonzero((r[:, 7] < 1) | (r[:, 7] >= program_rows))[0]
    _need(bad.size == 0, fn, "rows", f"row {int(bad[0]) if bad.size else 0} names program row {int(r[bad[0], 7]) if bad.size else 0}, outside 1 .. {program_rows - 1}")
    return torch.from_numpy(r.astype(np.int32)).to(device), torch.from_numpy(f.astype(np.int32)).to(device)


def note_levels(x, y, rows, out=None):
    """a2s_note_levels: x, y as for segment_agreement; rows: (S, 8) int32 on their device (note_table) -> (S, 3) float64 on the device, per row
    [sum x, sum y, count] over the cells of the row's partials (written into `out` when given)."""
    fn = "note_levels"
    x, y = _feature_pair(fn, x, y)
    B, T, F = x.shape
    _need(torch.is_tensor(rows) and rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == 8 and rows.is_contiguous() and rows.device == x.device,
          fn, "rows", "must be a contiguous int32 tensor (S, 8) on x's device")
    S = rows.shape[0]
    if out is None:
        out = torch.zeros((S, 3), dtype=torch.float64, device=x.device)
    _need(torch.is_tensor(out) and out.dtype == torch.float64 and tuple(out.shape) == (S, 3) and out.is_contiguous() and out.device == x.device, fn, "out",
          f"must be a contiguous float64 tensor ({S}, 3) on x's device")
    if S == 0:
        return out
    _need(B >= 1 and T >= 1 and F >= 1, fn, "x", f"has no cells (shape {tuple(x.shape)}) but the table has rows")
    check(lib().a2s_note_levels(stream(), _p(x), _p(y), _clip_stride(fn, x, y), B, T, F, _p(rows), S, _p(out)), "a2s_note_levels")
    return out


def note_amp_update(sums, rows, first, cum, programs, base_amp):
    """a2s_note_amp_update, in place: sums (S, 3) float64 of note_levels, rows (S, 8) and first (B + 1,) int32 of note_table (the table was checked
    there), cum (S,) float32, programs (B, 1 + E, 8) int32, all contiguous on one device.  Per clip: cum += the level difference, minus the clip's
    lower median, clamped to -30 .. 12 dB; the amplitude word of every listed program row becomes base_amp * 10^(cum / 20)."""
    fn = "note_amp_update"
    _need(torch.is_tensor(programs) and programs.dtype == torch.int32 and programs.dim() == 3 and programs.shape[2] == 8 and programs.shape[1] >= 2
          and programs.is_contiguous() and programs.is_cuda, fn, "programs", "must be contiguous int32 programs (B, 1 + E, 8) on the device")
    B, S = programs.shape[0], rows.shape[0] if torch.is_tensor(rows) else -1
    for name, t, dtype, shape in (("sums", sums, torch.float64, (S, 3)), ("rows", rows, torch.int32, (S, 8)), ("first", first, torch.int32, (B + 1,)),
                                  ("cum", cum, torch.float32, (S,))):
        _need(torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == programs.device, fn, name,
              f"must be a contiguous {dtype} tensor {shape} on the programs' device")
    _need(0.0 < float(base_amp) <= 1e30, fn, "base_amp", f"must be positive and finite (got {base_amp!r})")
    if S == 0 or B == 0:
        return cum
    check(lib().a2s_note_amp_update(stream(), _p(sums), _p(rows), _p(first), B, _p(cum), _p(programs), programs.shape[1], float(base_amp)), "a2s_note_amp_update")
    return cum


def dynamics_launches():
    """Launches of the two dynamics kernels in this process (a2s_dynamics_launches)."""
    return int(lib().a2s_dynamics_launches())


RETIME_N_MAX = 4096          # frames per segment a2s_path_warp takes (csrc/a2s_retime.hip)
RETIME_HOP_MAX = 65535       # the largest hop at which a2s_retime_events stays inside an int32


def _retime_table(fn, dev_table):
    _need(torch.is_tensor(dev_table) and dev_table.dtype == torch.int32 and dev_table.is_cuda and dev_table.dim() == 2 and dev_table.shape[1] == 4
          and dev_table.is_contiguous(), fn, "dev_table", "must be the contiguous int32 table (S, 4) on the device")
    return dev_table.shape[0]


def path_warp(paths, steps, dev_table, n_max, inverse=True):
    """a2s_path_warp: paths (S, L) int32 and steps (S,) int32 on the device as dtw_segments returns them, dev_table (S, 4) int32 [clip, f0, f1, r] on
    the same device, n_max >= the longest segment -> (warp2, inverse2), int32 (S, n_max + 1) each on the device (inverse2 None with inverse=False):
    twice resynth.warp_from_path, warp2[n] = warp2[n - 1] + 2, the identity 2 j behind n and for a path that is not one (include/a2s.h)."""
    fn = "path_warp"
    S = _retime_table(fn, dev_table)
    n_max = int(n_max)
    _need(1 <= n_max <= RETIME_N_MAX, fn, "n_max", f"must be in 1 .. {RETIME_N_MAX} (got {n_max})")
    _need(torch.is_tensor(paths) and paths.dtype == torch.int32 and paths.dim() == 2 and paths.shape[0] == S and paths.shape[1] >= 1 and paths.is_contiguous()
          and paths.device == dev_table.device, fn, "paths", f"must be a contiguous int32 tensor ({S}, L >= 1) on the table's device")
    _need(torch.is_tensor(steps) and steps.dtype == torch.int32 and tuple(steps.shape) == (S,) and steps.is_contiguous() and steps.device == dev_table.device,
          fn, "steps", f"must be a contiguous int32 tensor ({S},) on the table's device")
    warp2 = torch.empty((S, n_max + 1), dtype=torch.int32, device=dev_table.device)
    inverse2 = torch.empty_like(warp2) if inverse else None
    if S:
        check(lib().a2s_path_warp(stream(), _p(paths), paths.shape[1], _p(steps), _p(dev_table), S, n_max, _p(warp2), None if inverse2 is None else _p(inverse2)),
              "a2s_path_warp")
    return warp2, inverse2


def event_table(rows, n_clips, program_rows, table, device):
    """The HOST event table of a2s_retime_events, checked and uploaded once: rows (E, 5) or (E, 8) whole numbers [clip, prog_row, seg, bar_start,
    bar_stop(, 0, 0, 0)]; table: the HOST segment table (S, 3 or 4) [clip, f0, f1(, r)] the warps belong to.  Rows sorted by clip, 0 <= clip <
    n_clips, 1 <= prog_row < program_rows and no program row named twice (the kernel cannot refuse a row: it reads nothing back), seg = -1 (the event
    stays where it is) or a row of `table` of the same clip, everything an int32 -> (E, 8) int32 contiguous on `device`."""
    fn = "event_table"
    try:
        r, t = np.asarray(rows), np.asarray(table)
        whole = all(a.size == 0 or np.issubdtype(a.dtype, np.integer) or bool(np.all(a == np.rint(a))) for a in (r, t))
    except (TypeError, ValueError):
        r, t, whole = None, None, False
    _need(whole, fn, "rows", "and `table` must hold whole numbers")
    r = r.reshape(0, 8) if r.size == 0 else r
    t = t.reshape(0, 4) if t.size == 0 else t
    _need(r.ndim == 2 and r.shape[1] in (5, 8) and bool(np.all(np.abs(r.astype(np.int64)) < 2 ** 31)), fn, "rows", f"must be (E, 5) or (E, 8) int32 values (got {r.shape})")
    _need(t.ndim == 2 and t.shape[1] in (3, 4), fn, "table", f"must be (S, 3) or (S, 4) (got {t.shape})")
    r, t = r.astype(np.int64), t.astype(np.int64)
    S = t.shape[0]
    _need(int(n_clips) >= 1 and int(program_rows) >= 2, fn, "n_clips", f"and program_rows must be at least 1 and 2 (got {n_clips}, {program_rows})")
    _need(bool(np.all((r[:, 0] >= 0) & (r[:, 0] < n_clips) & (np.diff(r[:, 0], prepend=0) >= 0))), fn, "rows", f"must be sorted by clip, 0 <= clip < {n_clips}")
    bad = np.nonzero((r[:, 1] < 1) | (r[:, 1] >= program_rows))[0]
    _need(bad.size == 0, fn, "rows", f"row {int(bad[0]) if bad.size else 0} names program row {int(r[bad[0], 1]) if bad.size else 0}, outside 1 .. {int(program_rows) - 1}")
    _need(len(np.unique(r[:, 0] * int(program_rows) + r[:, 1])) == len(r), fn, "rows", "name a program row twice")
    seg = r[:, 2]
    fine = (seg >= -1) & (seg < S)
    listed = fine & (seg >= 0)
    fine[listed] = t[seg[listed], 0] == r[listed, 0]
    bad = np.nonzero(~fine)[0]
    _need(bad.size == 0, fn, "rows", f"row {int(bad[0]) if bad.size else 0} names segment {int(r[bad[0], 2]) if bad.size else 0}: neither -1 nor a row of the table of its clip")
    out = np.zeros((len(r), 8), dtype=np.int32)
    out[:, :5] = r[:, :5]
    return torch.from_numpy(out).to(device)


def retime_events(warp2, dev_table, events, hop, programs):
    """a2s_retime_events, in place: warp2 (S, n_max + 1) int32 of path_warp, dev_table (S, 4) int32, events (E, 8) int32 of event_table (checked
    there), programs (B, 1 + rows, 8) int32, all contiguous on one device.  Words 0 and 1 (onset, length) of every listed program row are moved
    through the warp of the row's segment (include/a2s.h); nothing else is written.  Returns programs."""
    fn = "retime_events"
    S = _retime_table(fn, dev_table)
    _need(torch.is_tensor(programs) and programs.dtype == torch.int32 and programs.dim() == 3 and programs.shape[2] == 8 and programs.shape[1] >= 2
          and programs.is_contiguous() and programs.device == dev_table.device, fn, "programs", "must be contiguous int32 programs (B, 1 + E, 8) on the table's device")
    _need(torch.is_tensor(warp2) and warp2.dtype == torch.int32 and warp2.dim() == 2 and warp2.shape[0] == S and 2 <= warp2.shape[1] <= RETIME_N_MAX + 1
          and warp2.is_contiguous() and warp2.device == dev_table.device, fn, "warp2", f"must be a contiguous int32 tensor ({S}, n_max + 1), n_max <= {RETIME_N_MAX}, on the table's device")
    _need(torch.is_tensor(events) and events.dtype == torch.int32 and events.dim() == 2 and events.shape[1] == 8 and events.is_contiguous()
          and events.device == dev_table.device, fn, "events", "must be a contiguous int32 tensor (E, 8) on the table's device")
    hop = int(hop)
    _need(1 <= hop <= RETIME_HOP_MAX, fn, "hop", f"must be in 1 .. {RETIME_HOP_MAX} (got {hop})")
    if S and events.shape[0] and programs.shape[0]:
        check(lib().a2s_retime_events(stream(), _p(warp2), warp2.shape[1] - 1, _p(dev_table), S, _p(events), events.shape[0], hop, _p(programs),
                                      programs.shape[0], programs.shape[1]), "a2s_retime_events")
    return programs


def retime_launches():
    """Launches of the two retiming kernels in this process (a2s_retime_launches)."""
    return int(lib().a2s_retime_launches())


TUNING_CELLS = 100           # histogram cells per semitone of the tuning kernels (csrc/a2s_tuning.hip): a row of hist holds TUNING_CELLS + 1 int64


def tuning_profile(x, n_rows, thr=0.5, bins_per_semitone=5, out=None):
    """a2s_tuning_profile: x (B, rows, F) or (B, 1, rows, F) float32 on the device, unit stride along F (the rows and the clips may be strided), n_rows
    (B,) int32 -> hist (B, 101) int64 on the device (written into `out` when given; overwritten): per clip the histogram of its spectral peaks'
    positions modulo one semitone, 100 cells of one cent each weighted by the peaks' heights, and in cell 100 the number of peaks."""
    fn = "tuning_profile"
    _need(torch.is_tensor(x) and x.dtype == torch.float32 and x.is_cuda and (x.dim() == 3 or (x.dim() == 4 and x.shape[1] == 1)), fn, "x",
          "must be a float32 tensor (B, rows, F) or (B, 1, rows, F) on the device")
    if x.dim() == 4:
        x = x[:, 0]
    B, rows, F = x.shape
    S, = _whole(fn, bins_per_semitone=bins_per_semitone)
    _need(1 <= S <= 64, fn, "bins_per_semitone", f"must be in 1 .. 64 (got {S})")
    try:
        t = float(thr)
    except (TypeError, ValueError):
        t = float("nan")
    _need(0.0 <= t <= 1.0, fn, "thr", f"must be a number in 0 .. 1 (got {thr!r})")
    _int_rows(fn, "n_rows", n_rows, (B,), x.device)
    if out is None:
        out = torch.zeros((B, TUNING_CELLS + 1), dtype=torch.int64, device=x.device)
    _need(torch.is_tensor(out) and out.dtype == torch.int64 and tuple(out.shape) == (B, TUNING_CELLS + 1) and out.is_contiguous() and out.device == x.device,
          fn, "out", f"must be a contiguous int64 tensor ({B}, {TUNING_CELLS + 1}) on x's device")
    if B == 0 or rows == 0 or F == 0:
        _need(B == 0 or F > 0 or rows == 0, fn, "x", "has rows but no columns")
        return out.zero_()
    _need(x.stride(2) == 1 or F == 1, fn, "x", "must have unit stride along F")
    xr = x.stride(1) if rows > 1 else max(x.stride(1), F)
    xb = x.stride(0) if B > 1 else max(x.stride(0), (rows - 1) * xr + F)
    _need(xr >= F and xb >= (rows - 1) * xr + F, fn, "x", f"has overlapping rows or clips (strides {tuple(x.stride())})")
    check(lib().a2s_tuning_profile(stream(), _p(x), xb, xr, _p(n_rows), B, rows, F, S, t, _p(out)), "a2s_tuning_profile")
    return out


def tuning_estimate(hist, first, min_conf, min_peaks, bins_per_semitone=5):
    """a2s_tuning_estimate: hist (B, 101) int64 on the device (tuning_profile); first: the groups' offsets, G + 1 whole numbers ascending from 0 to B
    -- the HOST table (anything numpy reads), checked here before it is uploaded, or an int32 tensor on hist's device that an earlier call checked
    (piano_a2s_amd.tuning.Tuner keeps one) -> (est (G, 3) float64 [cents, confidence, peaks], eff_bins (B,) float32: -cents * S / 100 for the
    clips of every group with at least min_peaks peaks and a confidence of at least min_conf, else 0), both on the device."""
    fn = "tuning_estimate"
    _need(torch.is_tensor(hist) and hist.dtype == torch.int64 and hist.dim() == 2 and hist.shape[1] == TUNING_CELLS + 1 and hist.is_contiguous() and hist.is_cuda,
          fn, "hist", f"must be a contiguous int64 tensor (B, {TUNING_CELLS + 1}) on the device")
    B = hist.shape[0]
    S, mp = _whole(fn, bins_per_semitone=bins_per_semitone, min_peaks=min_peaks)
    _need(1 <= S <= 64, fn, "bins_per_semitone", f"must be in 1 .. 64 (got {S})")
    _need(0 <= mp < 2 ** 31, fn, "min_peaks", f"must be in 0 .. 2^31 - 1 (got {mp})")
    try:
        mc = float(min_conf)
    except (TypeError, ValueError):
        mc = float("nan")
    _need(np.isfinite(mc), fn, "min_conf", f"must be a finite number (got {min_conf!r})")
    if torch.is_tensor(first) and first.is_cuda:
        _need(first.dtype == torch.int32 and first.dim() == 1 and first.numel() >= 1 and first.is_contiguous() and first.device == hist.device, fn, "first",
              "on the device must be a contiguous 1-D int32 tensor on hist's device")
    else:
        from .tuning import check_first
        try:
            table = check_first(first.cpu().numpy() if torch.is_tensor(first) else first, B)
        except ValueError as e:
            raise A2SError(f"{fn}: {e}") from None
        first = torch.from_numpy(table.astype(np.int32)).to(hist.device)
    G = first.numel() - 1
    _need(G <= 65535, fn, "first", f"names {G} groups, more than 65535")
    est = torch.zeros((G, 3), dtype=torch.float64, device=hist.device)
    eff = torch.zeros((B,), dtype=torch.float32, device=hist.device)
    if G == 0:
        return est, eff
    check(lib().a2s_tuning_estimate(stream(), _p(hist), _p(first), G, B, S, mc, mp, _p(est), _p(eff)), "a2s_tuning_estimate")
    return est, eff


def tuning_launches():
    """Kernel launches of the two tuning kernels in this process (a2s_tuning_launches)."""
    return int(lib().a2s_tuning_launches())


def agreement_launches():
    """Launches of the two agreement kernels in this process (a2s_agreement_launches)."""
    return int(lib().a2s_agreement_launches())


def agreement_partial_cells():
    """The most cells one fp32 partial sum of a2s_segment_agreement covers (a2s_agreement_partial_cells); everything above is added in double."""
    return int(lib().a2s_agreement_partial_cells())


def note_match(ref, ref_off, hyp, hyp_off, n_pairs, dur_ticks, midi, cls, out):
    """a2s_note_match: the note counts of n_pairs pairs of bar rows, one launch on the current stream.  ref / hyp (int32 ids) and ref_off / hyp_off
    (int64, n_pairs + 1 each) are device tensors or device addresses (ints: parts of one packed buffer, metrics.device_note_counts); dur_ticks, midi, cls
    the (V,) int32 tables of metrics.note_tables() on the device; out (n_pairs, 8) int32 receives the counts.  Returns out."""
    fn = "note_match"
    for name, t, dtype in (("ref", ref, torch.int32), ("hyp", hyp, torch.int32), ("ref_off", ref_off, torch.int64), ("hyp_off", hyp_off, torch.int64)):
        _need(isinstance(t, int) or (torch.is_tensor(t) and t.dtype == dtype and t.is_contiguous()), fn, name, f"must be a contiguous {dtype} tensor or an address")
    for name, t in (("ref_off", ref_off), ("hyp_off", hyp_off)):
        _need(isinstance(t, int) or t.numel() == n_pairs + 1, fn, name, f"must have n_pairs + 1 = {n_pairs + 1} elements")
    for name, t in (("dur_ticks", dur_ticks), ("midi", midi), ("cls", cls)):
        _need(torch.is_tensor(t) and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() == dur_ticks.numel(), fn, name,
              "must be a contiguous int32 tensor (V,)")
    _need(torch.is_tensor(out) and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == 8 * n_pairs, fn, "out",
          f"must be a contiguous int32 tensor of 8 * n_pairs = {8 * n_pairs} elements")
    if n_pairs == 0:
        return out
    check(lib().a2s_note_match(stream(), _p(ref), _p(ref_off), _p(hyp), _p(hyp_off), n_pairs, _p(dur_ticks), _p(midi), _p(cls), dur_ticks.numel(), _p(out)),
          "a2s_note_match")
    return out


def note_match_launches():
    """Launches of the note-matching kernel in this process (a2s_note_match_launches)."""
    return int(lib().a2s_note_match_launches())


def align_buffers(R, max_steps, T, device):
    """The outputs of one alignment call (a2s_align_args) over R rows: -> (AlignArgs, dict of the tensors it points to), pre-filled with what a step
    that never runs keeps: peak -1, weight 0, centroid -1."""
    t = dict(attw_step=torch.zeros((R, T), dtype=torch.float32, device=device),
             peak=torch.full((R, max_steps), -1, dtype=torch.int32, device=device),
             weight=torch.zeros((R, max_steps), dtype=torch.float32, device=device),
             centroid=torch.full((R, max_steps), -1.0, dtype=torch.float32, device=device))
    g = AlignArgs()
    for name in ("attw_step", "peak", "weight", "centroid"):
        setattr(g, name, t[name].data_ptr())
    g.out_stride = max_steps
    g.next_state, g.n_states, g.row_state = None, 0, None
    return g, t


def check(rc, what):
    if rc != 0:
        raise A2SError(f"{what} failed ({rc}): {lib().a2s_last_error().decode()}")


def f32(x):
    return C.c_float(float(x))


def gemm(A, sAm, sAk, B, sBk, sBn, Cout, ldc, M, N, K, alpha=1.0, beta=0.0, bias=None, act=0,
         batch=1, bsA=0, bsB=0, bsC=0, splitk=1, a_off=0, b_off=0, c_off=0, a_affine=None, b_affine=None, two_term=None):
    """C[m,n] = act(alpha*sum_k A(m,k)B(k,n) + beta*C + bias[n]); *_off are element offsets into the tensors.
    a_affine / b_affine = (scale, shift, period): BatchNorm+ReLU of that operand applied while it is staged (a2s_gemm_f32_affine).
    two_term = (a_absmax, b_absmax): device scalars max|A| / max|B| (None: the operand is O(1)) -- the product may run on the two-term
    fp16 split (a2s_gemm_f32_affine_scaled)."""
    L = lib()
    ws, ws_bytes = None, 0
    if splitk > 1:
        ws_bytes = L.a2s_gemm_workspace_bytes(M, N, batch, splitk)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=Cout.device)
    pa = C.c_void_p(A.data_ptr() + 4 * a_off)
    pb = C.c_void_p(B.data_ptr() + 4 * b_off)
    pc = C.c_void_p(Cout.data_ptr() + 4 * c_off)
    if a_affine is None and b_affine is None and two_term is None:
        check(L.a2s_gemm_f32(stream(), M, N, K, alpha, pa, sAm, sAk, pb, sBk, sBn, beta, pc, ldc, _p(bias), act, batch, bsA, bsB, bsC, splitk, _p(ws), ws_bytes),
              "a2s_gemm_f32")
        return
    asc, ash, ap = a_affine if a_affine is not None else (None, None, 0)
    bsc, bsh, bp = b_affine if b_affine is not None else (None, None, 0)
    if two_term is not None:
        check(L.a2s_gemm_f32_affine_scaled(stream(), M, N, K, alpha, pa, sAm, sAk, pb, sBk, sBn, beta, pc, ldc, _p(bias), act, batch, bsA, bsB, bsC, splitk, _p(ws),
                                           ws_bytes, _p(asc), _p(ash), ap, _p(bsc), _p(bsh), bp, _p(two_term[0]), _p(two_term[1])), "a2s_gemm_f32_affine_scaled")
        return
    check(L.a2s_gemm_f32_affine(stream(), M, N, K, alpha, pa, sAm, sAk, pb, sBk, sBn, beta, pc, ldc, _p(bias), act, batch, bsA, bsB, bsC, splitk, _p(ws), ws_bytes,
                                _p(asc), _p(ash), ap, _p(bsc), _p(bsh), bp), "a2s_gemm_f32_affine")


_ONES = {}


def one(device):
    """Device scalar 1.0: the range of an operand bounded by 1 (GRU states, softmax weights) for the two-term fp16 products."""
    key = torch.device(device).index
    if key not in _ONES:
        _ONES[key] = torch.ones(1, dtype=torch.float32, device=device)
    return _ONES[key]


def absmax(x, out=None):
    """max |x| of a contiguous float32 tensor as a device scalar (operand scale of the two-term fp16 kernels)."""
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().a2s_absmax(stream(), _p(x), x.numel(), _p(out)), "a2s_absmax")
    return out


def linear(x2d, weight, bias=None, act=0, out=None, beta=0.0, x_affine=None, two_term=None):
    """y = act(x @ weight.T + bias) for row-major contiguous x (M,K) and weight (N,K); x_affine = (scale, shift, period): the input
    is max(0, x*scale[k // period] + shift[k // period]) formed on the fly."""
    M, K = x2d.shape
    N = weight.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x2d.device)
    gemm(x2d, x2d.stride(0), x2d.stride(1), weight, weight.stride(1), weight.stride(0), out, out.stride(0), M, N, K,
         bias=bias, act=act, beta=beta, a_affine=x_affine, two_term=two_term)
    return out


# ---- the ConvStack's launches as the engine issues them (one place: engine.py / engine_bwd.py and the robustness tests share these)
def conv3x3_forward(x, w, y, scale, shift, partial, cws, in_absmax=None, out_absmax=None):
    """y = conv3x3(relu(x * scale[c] + shift[c])) (scale None: x as it is), (B, T, C, F) tensors; batch-statistics partials in `partial`;
    in_absmax / out_absmax: per-channel max |x| (from the launch that produced x) / max |y| (written here) -- a2s_conv3x3_ranged."""
    B, T, Cin, F = x.shape
    check(lib().a2s_conv3x3_ranged(stream(), _p(x), _p(w), _p(y), _p(scale), _p(shift), _p(in_absmax), _p(partial), _p(out_absmax),
                                   B, T, F, Cin, y.shape[2], _p(cws)), "a2s_conv3x3_ranged")


def conv3x3_dgrad_for_test(dy, w, yl):
    """Data gradient of a (Cin -> Cout) layer as engine_bwd issues it: dy (B, T, Cout, F) -> dx (B, T, Cin, F), operand scaled by the
    power of two derived from max|dy|, BatchNorm-backward statistics epilogue against `yl` (identity BatchNorm parameters here)."""
    (B, T, Cout, F), Cin, dev = dy.shape, w.shape[1], dy.device
    dx = torch.full((B, T, Cin, F), float("nan"), device=dev)
    part = torch.zeros(lib().a2s_conv3x3_stat_blocks(B, T, F, Cout), Cin, 2, device=dev)
    zeros, ones = torch.zeros(Cin, device=dev), torch.ones(Cin, device=dev)
    conv3x3_dgrad(dy, w, dx, conv_workspace(Cout, dev), (yl, (zeros, ones, ones, zeros), part), absmax(dy))
    torch.cuda.synchronize()
    return dx


def act_bound(scale, shift, x_absmax):
    """Device scalar bounding relu(x * scale[c] + shift[c]) over the tensor, from the per-channel max |x| its producer wrote."""
    out = torch.empty(1, dtype=torch.float32, device=scale.device)
    check(lib().a2s_act_bound(stream(), _p(scale), _p(shift), _p(x_absmax), scale.numel(), _p(out)), "a2s_act_bound")
    return out


def conv3x3_wgrad(dy, x, scale, shift, dW, ws, dy_absmax, act_absmax):
    """dW += weight gradient of a 3x3 layer from dy (B, T, Cout, F) and the layer input relu(x * scale + shift) (scale None: x as it is);
    dy_absmax / act_absmax: device scalars max |dy| / bound of the activated input (None: unknown -> that operand unscaled)."""
    B, T, Cout, F = dy.shape
    Cin = x.shape[2]
    check(lib().a2s_conv3x3_wgrad_ranged(stream(), _p(dy), _p(x), _p(scale), _p(shift), _p(dW), _p(ws), ws.numel() * 4, B, T, F, Cin, Cout, _p(dy_absmax),
                                         _p(act_absmax)), "a2s_conv3x3_wgrad_ranged")


def conv3x3_wgrad_for_test(dy, x, scale, shift):
    """Weight gradient as engine_bwd issues it: dW (Cout, Cin, 3, 3) from dy (B, T, Cout, F) and the layer input relu(x * scale + shift),
    with both operand ranges (max |dy|; the activation bound from the input's per-channel max)."""
    L = lib()
    B, T, Cout, F = dy.shape
    Cin = x.shape[2]
    dev = dy.device
    dW = torch.zeros(Cout, Cin, 3, 3, device=dev)
    ws = torch.empty(L.a2s_conv3x3_wgrad_workspace_bytes(Cin, Cout) // 4, device=dev)
    bound = act_bound(scale, shift, x.abs().amax(dim=(0, 1, 3)).contiguous())
    conv3x3_wgrad(dy, x, scale, shift, dW, ws, absmax(dy), bound)
    torch.cuda.synchronize()
    return dW


def linear_forward(x2d, weight, x_affine, x_bound, w_absmax, out=None):
    """The ConvStack's 19200 -> 256 Linear forward as the engine issues it: the kernel of its own (csrc/a2s_linear.hip: weight pre-split once,
    activations through a four-stage LDS ring) where the shape qualifies (hip.LINEAR_KERNELS / A2S_LINEAR_KERNELS=0: never), the generic two-term GEMM tile otherwise."""
    M, K = x2d.shape
    N = weight.shape[0]
    L = lib()
    period = x_affine[2]
    if (LINEAR_KERNELS and x2d.is_contiguous() and weight.is_contiguous() and x_bound is not None
            and L.a2s_linear_fwd_eligible(M, N, K, period)):
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=x2d.device)
        nb = L.a2s_linear_dgrad_ws_bytes(N, K)
        ws = torch.empty(nb // 4, dtype=torch.float32, device=x2d.device)
        check(L.a2s_linear_fwd(stream(), M, N, K, _p(x2d), K, _p(weight), _p(out), N, _p(x_affine[0]), _p(x_affine[1]), period, _p(x_bound), _p(w_absmax), _p(ws), nb),
              "a2s_linear_fwd")
        return out
    return linear(x2d, weight, out=out, x_affine=x_affine, two_term=(x_bound, w_absmax))


def linear_forward_f64(x2d, weight, x_affine):
    """The same Linear with products and sums in double (a2s_linear_fwd_f64): what Engine.convstack takes in a training call of at most 64 rows."""
    M, K = x2d.shape
    out = torch.empty((M, weight.shape[0]), dtype=torch.float32, device=x2d.device)
    check(lib().a2s_linear_fwd_f64(stream(), M, weight.shape[0], K, _p(x2d), _p(weight), _p(out), _p(x_affine[0]), _p(x_affine[1]), x_affine[2]), "a2s_linear_fwd_f64")
    return out


def linear_wgrad(dz, x2d, x_affine, dz_absmax, x_bound, G):
    """G (N, K) += dz^T relu(bn(x)) for the ConvStack's 19200 -> 256 Linear on the kernel of csrc/a2s_linear.hip; returns False when the shape
    does not qualify (hip.LINEAR_KERNELS off: never) -- the caller then runs the generic split-K GEMM."""
    M, K = x2d.shape
    N = dz.shape[1]
    L = lib()
    if (not LINEAR_KERNELS or not (x2d.is_contiguous() and dz.is_contiguous() and G.is_contiguous()) or dz_absmax is None
            or x_bound is None or not L.a2s_linear_wgrad_eligible(M, N, K, x_affine[2])):
        return False
    nb = L.a2s_linear_wgrad_ws_bytes(M, K)
    ws = torch.empty(nb // 4, dtype=torch.float32, device=x2d.device)
    check(L.a2s_linear_wgrad(stream(), M, N, K, _p(dz), N, _p(x2d), K, _p(G), K, _p(x_affine[0]), _p(x_affine[1]), x_affine[2], _p(dz_absmax), _p(x_bound), _p(ws), nb),
          "a2s_linear_wgrad")
    return True


# ---- the ConvStack backward's launches as engine_bwd._convstack_bwd issues them (conv_bwd_plan.py says when).  bn = (mean, invstd, scale, shift); dims = (rows,
# channels, F); dgamma / dbeta accumulate; every BatchNorm backward returns c12, its two per-channel means; mask: dropout (kept elements scaled by 1 / 0.8)
def _f32(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def bn_bwd(g, x, bn, mask, dgamma, dbeta, dx, dims, amax, partial=None):
    """dx (None: statistics only; g: in place) and max |dx| into amax; statistics by a pass of its own, or from partial = (tensor, blocks) of g's producer."""
    c12 = _f32(g, 2 * dims[1])
    if partial is None:
        part = _f32(g, lib().a2s_bn_bwd_partial_floats(*dims))
        check(lib().a2s_bn_bwd_amax(stream(), _p(g), _p(x), *map(_p, bn), _p(mask), 1.0 / 0.8, _p(dgamma), _p(dbeta), _p(dx), _p(part), _p(c12), *dims, _p(amax)),
              "a2s_bn_bwd")
    else:
        check(lib().a2s_bn_bwd_from_partial_amax(stream(), _p(g), _p(x), *map(_p, bn), _p(dgamma), _p(dbeta), _p(dx), _p(partial[0]), partial[1], _p(c12), *dims,
                                                 _p(amax)), "a2s_bn_bwd_from_partial")
    return c12


def bn_bwd_sync(g, x, bn, mask, dgamma, dbeta, dims, count, all_reduce, partial=None):
    """Synchronised: this rank's sums (partial None: by a pass, and dx over g in place; else from the partials, statistics only) and ONE small all-reduce."""
    L, local, c12 = lib(), _f32(g, 2 * dims[1]), _f32(g, 2 * dims[1])
    if partial is None:
        part = _f32(g, L.a2s_bn_bwd_partial_floats(*dims))
        check(L.a2s_bn_bwd_stats(stream(), _p(g), _p(x), *map(_p, bn), _p(mask), 1.0 / 0.8, _p(part), _p(local), *dims), "a2s_bn_bwd_stats")
    else:
        check(L.a2s_bn_bwd_sums_from_partial(stream(), _p(partial[0]), partial[1], dims[1], _p(local)), "a2s_bn_bwd_sums_from_partial")
    glob = local.clone()
    all_reduce(glob)
    if partial is None:
        check(L.a2s_bn_bwd_apply(stream(), _p(g), _p(x), *map(_p, bn), _p(mask), 1.0 / 0.8, _p(local), _p(glob), count, _p(dgamma), _p(dbeta), _p(g), _p(c12), *dims),
              "a2s_bn_bwd_apply")
    else:
        check(L.a2s_bn_bwd_c12_from_sums(stream(), _p(local), _p(glob), count, _p(dgamma), _p(dbeta), _p(c12), dims[1]), "a2s_bn_bwd_c12_from_sums")
    return c12


def conv3x3_wgrad_bn(g, y, bn, c12, dy, x, in_bn, dW, ws, ranged=None):
    """dW (Cout, Cin, 3, 3) += weight gradient by a kernel that forms dy from (g, y, c12) itself; in_bn: of the layer below (None: x as it is).  ranged None:
    tiled, dy (None: not needed) written out; (g_absmax, y_absmax, dy_absmax out, act_absmax): row-streaming, dy over g IN PLACE (LayerPlan.form)."""
    B, T, _, F = g.shape
    sc, sh = in_bn[2:] if in_bn else (None, None)
    tail = _p(x), _p(sc), _p(sh), _p(dW), _p(ws), ws.numel() * 4, B, T, F, dW.shape[1], dW.shape[0]
    if ranged is None:
        return check(lib().a2s_conv3x3_wgrad_bn(stream(), _p(g), _p(y), *map(_p, bn), _p(c12), _p(dy), *tail), "a2s_conv3x3_wgrad_bn")
    g_absmax, y_absmax, dy_absmax, act_absmax = ranged
    check(lib().a2s_conv3x3_wgrad_bn_ranged(stream(), _p(g), _p(y), *map(_p, bn), _p(c12), _p(g_absmax), g_absmax.numel(), _p(y_absmax), _p(g), _p(dy_absmax), *tail,
                                            _p(act_absmax)), "a2s_conv3x3_wgrad_bn_ranged")


def conv3x3_dgrad(dy, w, dx, cws, below=None, dy_absmax=None, out_absmax=None):
    """dx (B, T, Cin, F) = data gradient for weight w (Cout, Cin, 3, 3): plain, or with below = (y, bn, partial out) of the layer below its statistics
    partials in the epilogue, operand scaled by max |dy| (dy_absmax; None: unscaled), per-channel max |dx| into out_absmax if given (LayerPlan.dgrad)."""
    B, T, _, F = dy.shape
    if below is None:
        return check(lib().a2s_conv3x3(stream(), _p(dy), _p(w), _p(dx), None, None, None, B, T, F, w.shape[0], w.shape[1], 1, _p(cws)), "a2s_conv3x3 dgrad")
    check(lib().a2s_conv3x3_dgrad_bnstats_ranged(stream(), _p(dy), _p(w), _p(dx), _p(below[0]), *map(_p, below[1]), _p(below[2]), B, T, F, w.shape[0], w.shape[1],
                                                 _p(cws), _p(dy_absmax), _p(out_absmax)), "a2s_conv3x3_dgrad_bnstats")


def linear_dgrad_bnstats(dz, W, da, y, bn, F, dz_absmax, w_absmax, own):
    """da (rows, K) = dz W of the ConvStack's Linear, layer 4's BatchNorm-backward statistics (y, bn; column k is channel k // F) in the epilogue; own:
    the kernel of csrc/a2s_linear.hip, else the generic GEMM tiles (LinearPlan.dgrad).  Returns ((partials, blocks), max |da| or None)."""
    L, (rows, Cf), K = lib(), dz.shape, W.shape[1]
    nblk = L.a2s_linear_dgrad_blocks(rows) if own else L.a2s_gemm_bnstats_blocks(rows, F)
    part = _f32(dz, nblk, K // F, 2)
    if own:
        nb = L.a2s_linear_dgrad_ws_bytes(K, Cf)
        Wt, ws, amax = W.t().contiguous(), _f32(dz, nb // 4), torch.zeros(1, dtype=torch.float32, device=dz.device)
        check(L.a2s_linear_dgrad_bnstats(stream(), rows, K, Cf, _p(dz), Cf, _p(Wt), _p(da), K, _p(y), *map(_p, bn), F, _p(part), _p(dz_absmax), _p(w_absmax), _p(ws), nb,
                                         _p(amax)), "a2s_linear_dgrad_bnstats")
        return (part, nblk), amax
    # a k-contiguous copy of the weight (19.7 MB) puts this product on the split-operand path of the GEMM (both operands k-contiguous)
    wb, s_bk, s_bn = (W.t().contiguous(), 1, Cf) if L.a2s_debug_get(b"gemm_bf16x3") > 0 else (W, K, 1)
    check(L.a2s_gemm_f32_bnstats_scaled(stream(), rows, K, Cf, _p(dz), Cf, 1, _p(wb), s_bk, s_bn, _p(da), K, _p(y), *map(_p, bn), F, _p(part), _p(dz_absmax), _p(w_absmax)),
          "a2s_gemm_f32_bnstats_scaled")
    return (part, nblk), None


_TALLK_WS = {}


def tallk_wgrad(P, p_off, ldp, A, a_off, lda, G, g_off, ldg, M, Np, K, p_absmax, a_absmax, transposed=False, bias=None):
    """G (+)= P^T A over M rows on the tall-K kernel of csrc/a2s_linear.hip (a2s_tallk_wgrad): P (M, Np) is packed, A (M, K) streamed once; *_off
    are element offsets into the tensors, ld* their row strides.  transposed: the result lands as G[k][n].  bias: bias[k] += column sums of A.
    Returns False when the shape does not qualify or the switch "tallk_wgrad" is off -- the caller then runs the generic split-K GEMM.
    The workspace (operand planes + slabs) is kept per (device, stream, host thread): steady-state steps allocate nothing."""
    L = lib()
    if not hasattr(L, "a2s_tallk_wgrad_eligible"):
        return False
    pp, pa, pg = P.data_ptr() + 4 * p_off, A.data_ptr() + 4 * a_off, G.data_ptr() + 4 * g_off
    if (p_absmax is None or a_absmax is None or (pp | pa | pg | (bias.data_ptr() if bias is not None else 0)) % 16
            or not L.a2s_tallk_wgrad_eligible(M, Np, K, ldp, lda, ldg, int(transposed))):
        return False
    nb = L.a2s_tallk_wgrad_ws_bytes(M, Np, K)
    key = (A.device, torch.cuda.current_stream().cuda_stream, threading.get_ident())
    ws = _TALLK_WS.get(key)
    if ws is None or ws.numel() * 4 < nb:
        ws = _TALLK_WS[key] = torch.empty((nb + 3) // 4, dtype=torch.float32, device=A.device)
    check(L.a2s_tallk_wgrad(stream(), M, Np, K, C.c_void_p(pp), ldp, C.c_void_p(pa), lda, C.c_void_p(pg), ldg, int(transposed), _p(bias), _p(p_absmax), _p(a_absmax),
                            _p(ws), ws.numel() * 4), "a2s_tallk_wgrad")
    return True


def linear_forward_for_test(x, w, aff):
    """The 19200 -> 256 Linear's forward as engine.convstack issues it (operand BatchNorm+ReLU while staging, two-term split with the
    activation bound and max |w| as operand ranges)."""
    period = aff[2]
    xmax = x.view(x.shape[0], -1, period).abs().amax(dim=(0, 2)).contiguous()
    return linear_forward(x, w, aff, act_bound(aff[0], aff[1], xmax), absmax(w))
