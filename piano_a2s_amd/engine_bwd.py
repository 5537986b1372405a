"""Backward pass of the transcription model on liba2s_hip.so: the manual reverse of piano_a2s_amd.engine.Engine.forward.

What torch.autograd would compute for the reference graph (models.py:26-51 and everything below it), composed from
the C-ABI backward kernels.  Sequential parts (note-decoder steps, encoder GRU steps) run in C++ loops; everything that
does not depend on the recurrence is deferred and batched over all steps of a (bar, staff):
  * output projection: ONE GEMM for dlogits_all W_out and ONE for dW_out,
  * GRU / attention-query weight gradients: ONE GEMM each over all steps,
  * attention key/value side: dEnc via a kernel over the live (step, bar) pairs (or a batched (T x steps)(steps x 2H) GEMM), dK via a
    tanh-recompute kernel.
"""
import ctypes as C
import os
import threading
from collections import namedtuple

import torch

from . import hip
from .conv_bwd_plan import CHANS, ConvBwdFlags, plan_convstack_bwd
from .dec_bwd_plan import dim, plan_note_decoder_bwd, plan_staff_issue
from .spec import SOS, VOCAB_SIZE


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


_COLSUM_WS = {}


def _colsum(x, ld, out, rows, ncol, x_off=0, out_off=0, beta=1.0):
    ws = None
    if rows >= 2048:                                  # two-stage reduction scratch, one buffer per (device, stream), reused
        # (per host thread as well: two threads may issue into ONE stream -- engine.staff_streams -- and a reduction's two launches must
        # not be interleaved with another reduction that uses the same scratch)
        key = (x.device, torch.cuda.current_stream().cuda_stream, threading.get_ident())
        ws = _COLSUM_WS.get(key)
        if ws is None or ws.numel() < 1024 * ncol:
            ws = _COLSUM_WS[key] = torch.empty(1024 * max(ncol, 2048), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().a2s_col_sum(hip.stream(), _ptr(x, x_off), ld, _ptr(out, out_off), rows, ncol, 1.0, beta, hip._p(ws), ws.numel() if ws is not None else 0),
              "a2s_col_sum")


def _linear_bwd(x, W, dy, G, wname, bname, dx=None, dx_beta=0.0, x_affine=None, dy_amax=None, x_bound=None):
    """y = x W^T + b  (x (M,K) contiguous, W (N,K)):  dW += dy^T x ; db += colsum(dy) ; dx (+)= dy W.
    x_affine = (scale, shift, period): the layer's input was max(0, x*scale[k // period] + shift[k // period]) formed on the fly
    (hip.linear) -- the weight gradient re-forms it the same way while staging x.  dy_amax: device scalar max|dy| -- the weight
    gradient may then run on the two-term fp16 split (x is O(1): post-BatchNorm activations)."""
    M, K = x.shape
    N = W.shape[0]
    sk = hip.lib().a2s_gemm_pick_splitk(N, K, M, 1)
    hip.gemm(dy, 1, N, x, K, 1, G[wname], K, N, K, M, beta=1.0, splitk=sk, b_affine=x_affine, two_term=(dy_amax, x_bound) if dy_amax is not None else None)
    if bname is not None:
        _colsum(dy, N, G[bname], M, N)
    if dx is not None:
        hip.gemm(dy, N, 1, W, K, 1, dx, dx.stride(0), M, K, N, beta=dx_beta)
    return dx


def _staff_token_bwd(eng, S, G, rec, dtok):
    """Backward of one _staff_token call; dtok: (R, >= col0+2S) gradient buffer holding the token gradient."""
    L = hip.lib()
    names = [f"decoder.staff_emb.{w}_{sfx}" for sfx in ("l0", "l0_reverse") for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    warr = (C.c_void_p * 8)(*[S[n].data_ptr() for n in names])
    gptrs = G.get("__staff_emb_ptrs__")
    if gptrs is None:
        gptrs = torch.tensor([G[n].data_ptr() for n in names], dtype=torch.int64, device=dtok.device)
    E, Sz = eng.cfg["note_emb_size"], eng.cfg["staff_emb_size"]
    ids = rec["ids"]
    hip.check(L.a2s_staff_emb_bwd(hip.stream(), hip._p(S["decoder.note_emb.weight"]), warr, hip._p(gptrs), hip._p(G["decoder.note_emb.weight"]),
                                  hip._p(ids) if rec["i64"] else None, None if rec["i64"] else hip._p(ids), rec["id_bstride"], hip._p(rec["lengths"]), rec["len_stride"],
                                  hip._p(dtok), dtok.stride(0), rec["col0"], hip._p(rec["hsave"]), dtok.shape[0], rec["maxlen"], E, Sz), "a2s_staff_emb_bwd")
    return gptrs     # keep alive until the caller returns


def _attn_deferred(eng, S, G, prefix, keys, enc, q_all, ds_all, attw_all, dctx_all, dK, dEnc, B, T, H, steps, active=None, groups=1):
    """Key/value side of `steps` attention calls of one layer: dEnc += A^T dCtx (per clip), dK += ..., dv += ...
    The per-step tensors hold groups*B rows per step, row = group*B + clip (fused bars): (step, group) is one flat reduction index."""
    L = hip.lib()
    # dEnc[b] += sum_{s,g} a_sg[b,:]^T dctx_sg[b,:]   -- batched over clips: (T x steps*groups)(steps*groups x 2H)
    # (operand ranges for the two-term fp16 product: softmax weights <= 1, max |dctx| measured; K = steps * groups < 256 runs fp32-input)
    until = active["until"] if active else None
    if (2 * H == 512 and L.a2s_debug_get(b"attn_deferred_fast") > 0 and hasattr(L, "a2s_attn_denc_accum")
            and attw_all.is_contiguous() and dctx_all.is_contiguous() and dEnc.is_contiguous()):
        # ... on the kernel that walks only the clip's live pairs (fp32 matrix instructions: no operand range, no pass over dctx_all)
        hip.check(L.a2s_attn_denc_accum(hip.stream(), hip._p(attw_all), hip._p(dctx_all), hip._p(dEnc), B, T, steps, 2 * H, hip._p(until), groups),
                  "a2s_attn_denc_accum")
    else:
        hip.gemm(attw_all, 1, B * T, dctx_all, B * 2 * H, 1, dEnc, 2 * H, T, 2 * H, steps * groups, beta=1.0, batch=B, bsA=T, bsB=2 * H, bsC=T * 2 * H,
                 two_term=(hip.one(enc.device), hip.absmax(dctx_all)) if dctx_all.is_contiguous() else None)
    nblk = L.a2s_attn_dk_blocks(B, T)
    dvp = torch.empty((nblk, H), dtype=torch.float32, device=enc.device)
    hip.check(L.a2s_attn_dk_accum(hip.stream(), hip._p(keys), hip._p(q_all), hip._p(ds_all), hip._p(S[prefix + ".v.weight"]), hip._p(dK),
                                  hip._p(dvp), B, T, steps, H, hip._p(until), groups), "a2s_attn_dk_accum")
    _colsum(dvp, H, G[prefix + ".v.weight"], nblk, H)


def _consumed_tokens(sv, n, B, n_clips, dev):
    """(n, B) int32, the token each executed step consumed: <sos> at step 0, then the ground truth (where the row's group was teacher-forced) or the
    argmax of the previous step."""
    tok = torch.full((n, B), SOS, dtype=torch.int32, device=dev)
    if n > 1:
        prev = sv["ids"][:, :n - 1].t()
        if sv["gt_bar"] is not None:
            bits = sv.get("flags_dev")                                                                            # bit g: group g teacher-forced
            if bits is None:
                bits = torch.tensor(sv["flags"][:n - 1], dtype=torch.int32, device=dev)
            bits = bits[:n - 1].unsqueeze(1)
            grp = (torch.arange(B, dtype=torch.int32, device=dev) // n_clips).unsqueeze(0)
            prev = torch.where(((bits >> grp) & 1).bool(), sv["gt_bar"][:, :n - 1].t().to(torch.int32), prev)
        tok[1:] = prev
    return tok


def _dec_weight_side(plan, t, S, G, prefix, n, H, E):
    """The "weights" side of dec_bwd_plan: the products of plan.products over plan.rw rows, each with its bias sum.  t: the call's tensors by the plan's names."""
    L, dev, R = hip.lib(), t["dlog"].device, n * t["dlog"].shape[1]
    # operand ranges (two-term fp16 split): the bounds of the inputs as Product.x_bound states them, the gradients' max magnitudes measured
    one = hip.one(dev)
    bound = {"max(emb, enc)": torch.maximum(hip.absmax(S[prefix + ".embedding.weight"]), t["enc_amax"]), "max(one, enc)": torch.maximum(one, t["enc_amax"]), "one": one}
    if plan.empty:
        return
    rows = {k: (t[k] if t[k].shape[0] == n else t[k][:n]).view(R, t[k].shape[-1]) for k in plan.operands}          # (x, h: one row more than the executed steps)
    if plan.gather:          # the pairs that ran, as dense operands: the products, bias sums and measured ranges run over those only
        rows = {k: v.index_select(0, t["live_idx"]) for k, v in rows.items()}
    for p in plan.products:
        x, dy = rows[p.x], rows[p.dy]
        N, K = dy.shape[1], dim(p.cols, H, E)
        dy_amax = hip.absmax(dy) if p.dy_range == "measure" else t[p.dy_range]
        sk = L.a2s_gemm_pick_splitk(N, K, plan.rw, 1)
        hip.gemm(dy, 1, N, x, K, 1, G[prefix + p.weight], dim(p.ld, H, E), N, K, plan.rw, beta=1.0, splitk=sk, c_off=p.col0, two_term=(dy_amax, bound[p.x_bound]))
        _colsum(dy, N, G[prefix + p.bias], plan.rw, N)


def _dec_scatter(plan, t, sv, G, prefix, n, n_clips, E):
    """The "scatter" side: the embedding rows of the tokens consumed at each step (at the pairs that ran: their tokens, dx columns and dropout masks)."""
    dx, drop = t["dx"], t["drop"]
    B, ldx = dx.shape[1], dx.shape[2]
    tok, dx_w, ld_w = _consumed_tokens(sv, n, B, n_clips, dx.device), dx, ldx
    if plan.gather:
        tok = tok.view(-1).index_select(0, t["live_idx"])
        dx_w, ld_w = dx.view(n * B, ldx)[:, :E].index_select(0, t["live_idx"]), E
        if drop is not None:
            drop = drop.reshape(-1, E)[:n * B].index_select(0, t["live_idx"])
    hip.check(hip.lib().a2s_embed_scatter_add(hip.stream(), hip._p(G[prefix + ".embedding.weight"]), None, hip._p(tok), 1, 0, hip._p(dx_w), ld_w, 0, plan.rw, E, hip._p(drop),
                                              1.0 / (1.0 - sv["drop_p"]) if drop is not None else 1.0), "a2s_embed_scatter_add")


def _note_dec_bwd_args(S, sv, keys, enc, do_all, n_clips, T, H, E):
    """The argument block of a2s_note_decoder_bwd for one call, what the reverse loop writes allocated.  Returns (block, the tensors it writes by the
    names of dec_bwd_plan, the persistent launch's workspace or None: alive until the launch is enqueued)."""
    n, B, _ = do_all.shape
    H2, prefix, dev = 2 * H, sv["prefix"], enc.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    # (with m_active the per-step products skip the rows of finished clips: their dx rows are never written and must read as zero: zero-filled by the call)
    w = dict(dgi=new(n, B, 3 * H2), dgh=new(n, B, 3 * H2), dq=new(n, B, H), ds=new(n, B, T), dctx=new(n, B, H2), dx=new(n, B, E + H2), dh=new(2, B, H2))
    a = hip.NoteDecBwdArgs()
    for name, t in (("attn_w", S[prefix + ".attn.attn.weight"]), ("attn_v", S[prefix + ".attn.v.weight"]), ("w_ih", S[prefix + ".gru.weight_ih_l0"]),
                    ("w_hh", S[prefix + ".gru.weight_hh_l0"]), ("keys", keys), ("enc", enc), ("h", sv["h"]), ("x", sv["x"]), ("q", sv["q"]),
                    ("gates", sv["gates"]), ("attw", sv["attw"]), ("do_all", do_all), ("dgi_all", w["dgi"]), ("dgh_all", w["dgh"]),
                    ("dq_all", w["dq"]), ("ds_all", w["ds"]), ("dctx_all", w["dctx"]), ("dx", w["dx"]), ("dh", w["dh"]), ("attn_ws", sv["attn_ws"]), ("gemm_ws", sv["gemm_ws"])):
        setattr(a, name, t.data_ptr() if t is not None else None)
    a.gemm_ws_bytes = sv["gemm_ws"].numel() * 4 if sv["gemm_ws"] is not None else 0
    if sv.get("step_ws") is not None:
        a.step_ws, a.step_ws_floats = sv["step_ws"].data_ptr(), sv["step_ws"].numel()
    hip.set_row_plan(a, sv.get("active"))
    a.R, a.T, a.H, a.E, a.steps = B, T, H, E, n
    # the forward ran this call as one persistent launch (at most 8 clips): so does the reverse loop (csrc/a2s_dec_persist.hip)
    a.persist_ws, a.persist_ws_bytes, a.w_ih_full = None, 0, None
    persist_ws = None
    if sv.get("persist_ws") is not None:
        nb_ws = hip.lib().a2s_note_decoder_bwd_persist_ws_bytes(n_clips)
        if nb_ws:
            persist_ws = torch.empty(nb_ws, dtype=torch.uint8, device=dev)
            a.persist_ws, a.persist_ws_bytes = persist_ws.data_ptr(), nb_ws
    return a, w, persist_ws


def _note_decoder_bwd(eng, S, G, sv, keys, enc, dprobs_bar, probs_bar, dK, dEnc, n_clips, T, enc_amax, late=None, defer_launch=False):
    """Reverse of Engine._decode_staff.  Returns the gradient wrt the initial hidden (rows, 2H); rows = groups * n_clips.  enc_amax: device scalar max |enc|.
    What follows the reverse loop is dec_bwd_plan.plan_note_decoder_bwd's: this function allocates, launches and walks it.
    late: optional list.  The call's WEIGHT gradients (output projection, GRU, attention query half, embedding rows: everything only the
    optimizer waits for) are then not computed here: a (closure, event, tensors) entry is appended and Backward.finish runs the closures on the
    weight-gradient stream beside the encoder's back-propagation -- on the staff's own stream they sit in series with the next segment's decode
    steps (8-12 ms of GEMMs per call of the bulk clip group, profiles/r05_queue_timeline.txt).  The key / encoder-output gradients stay here.
    defer_launch (_note_decoder_bwd_pair): nothing is launched; returns (argument block, the rest of this function, what the launch needs alive)."""
    L = hip.lib()
    groups = sv.get("groups", 1)
    B = groups * n_clips
    H, E, V = eng.cfg["hidden_size"], eng.cfg["note_emb_size"], VOCAB_SIZE
    H2 = 2 * H
    n, prefix, dev = sv["steps"], sv["prefix"], enc.device
    R = n * B
    act = sv.get("active") or {}
    live = act.get("live_idx")
    plan = plan_note_decoder_bwd(n, B, act.get("live_steps"), live.numel() if live is not None else None, late is not None)
    # (a) dlogits for all executed steps, step-major (n, B, V)
    dlog = torch.empty((n, B, V), dtype=torch.float32, device=dev)
    hip.check(L.a2s_log_softmax_bwd_rows(hip.stream(), hip._p(dprobs_bar), hip._p(probs_bar), probs_bar.stride(0), n, hip._p(dlog), R, V, B, 1),
              "a2s_log_softmax_bwd_rows")
    # (b) the half of the output projection that gates the recurrence, all steps at once: do_all = dlog W_out
    do_all = torch.empty((n, B, 2 * H2), dtype=torch.float32, device=dev)
    Wo = S[prefix + ".out.weight"]
    dlog_amax = hip.absmax(dlog)
    hip.gemm(dlog.view(R, V), V, 1, Wo, 2 * H2, 1, do_all.view(R, 2 * H2), 2 * H2, R, 2 * H2, V, two_term=(dlog_amax, hip.absmax(Wo)))
    # (c) reverse recurrence
    a, w, persist_ws = _note_dec_bwd_args(S, sv, keys, enc, do_all, n_clips, T, H, E)
    if not defer_launch:
        hip.check(L.a2s_note_decoder_bwd(hip.stream(), C.byref(a)), "a2s_note_decoder_bwd")
    # (d) everything nobody in the recurrence waits for
    t = dict(w, dlog=dlog, do_all=do_all, dlog_amax=dlog_amax, enc_amax=enc_amax, live_idx=live, flags_dev=sv.get("flags_dev"),
             **{k: sv[k] for k in ("o", "x", "h", "ids", "drop", "gt_bar")})
    sides = {"weights": lambda: _dec_weight_side(plan, t, S, G, prefix, n, H, E),
             "keys": lambda: _attn_deferred(eng, S, G, prefix + ".attn", keys, enc, sv["q"], w["ds"], sv["attw"], w["dctx"], dK, dEnc, n_clips, T, H, n, sv.get("active"), groups),
             "scatter": lambda: _dec_scatter(plan, t, sv, G, prefix, n, n_clips, E)}

    def walk():
        for side in plan.on_stream:
            sides[side]()
        if plan.in_closure:
            ev = torch.cuda.Event()
            ev.record()
            # the entry holds everything the closure reads that was allocated on this (staff / group) stream: the weight-gradient stream records them all
            late.append((lambda: [sides[side]() for side in plan.in_closure], ev, tuple(t[k] for k in plan.keep_alive)))
        return w["dh"][0]

    if defer_launch:                  # the arguments are ready (kept alive by the closure), the caller launches both staves with one call
        return a, walk, (persist_ws,)
    return walk()


def _note_decoder_bwd_pair(calls, streams, pair):
    """The reverse loops of a segment's two note decoders issued by ONE host loop on their two streams (Engine._decode_pair in reverse): while both staves
    step, the attention sweep of a step is one launch that reads the encoder outputs once for both (a2s_note_decoder_bwd_pair).  calls: the argument
    tuples of _note_decoder_bwd (upper, lower); returns their results."""
    prepared = []
    for st, args in zip(streams, calls):
        with torch.cuda.stream(st):
            prepared.append(_note_decoder_bwd(*args, defer_launch=True))
    hip.check(hip.lib().a2s_note_decoder_bwd_pair(C.c_void_p(streams[0].cuda_stream), C.c_void_p(streams[1].cuda_stream), C.byref(prepared[0][0]),
                                                  C.byref(prepared[1][0]), hip._p(pair["order"]), hip._p(pair["rank"]), pair["n_active"]), "a2s_note_decoder_bwd_pair")
    res = []
    for st, (_, after, _keep) in zip(streams, prepared):
        with torch.cuda.stream(st):
            res.append(after())
    return res


class Backward:
    """The backward pass in three phases, so that the decoder part of each clip group can be started by whoever has that group's loss
    gradients first (train.TrainStep chains it right behind the group's forward, on the group's own streams):
        ctx = Backward(eng, S, (B, T, F), device, clip_groups, concurrent, bar_major)     allocations, before any group starts
        ctx.decoder_group(gidx, gs, dts_g, dkey_g, dup_g, dlo_g)                        one group: note decoders, bar chain, heads
        G = ctx.finish(grad_ready)                                                      keys, encoder, ConvStack
    What the groups write per CLIP (dEnc, dK, d_hidden) they write to disjoint slices; what they ACCUMULATE over clips (every weight
    gradient) goes to a flat gradient buffer of the group's own (16.4 M floats), added to `flat` once after the join -- no two streams
    ever accumulate into the same memory."""

    check_fold = False          # tests set it: finish() then verifies (with a host sync) what the late fold of the group buffers assumes

    def __init__(self, eng, S, shape, dev, clip_groups, concurrent, bar_major):
        from .spec import flat_layout, is_buffer
        self.eng, self.S, self.dev = eng, S, dev
        self.B, self.T, self.F = shape
        B, T = self.B, self.T
        H = eng.cfg["hidden_size"]
        H2 = 2 * H
        self.names = [k for k in S if not is_buffer(k)]
        self.offs, self.total = flat_layout([S[k].numel() for k in self.names])          # same layout as models.ScoreTranscription.flatten_()
        # one word behind the gradients: the step's loss (train.TrainStep writes it before finish()).  It rides in the FIRST slice that is
        # all-reduced, so the data-parallel skip / apply decision ("is every rank's loss finite?") needs no collective of its own.
        self.flat_full = torch.zeros(self.total + 1, dtype=torch.float32, device=dev)
        self.flat = self.flat_full[:self.total]
        self.G = {k: self.flat[off:off + S[k].numel()].view(S[k].shape) for k, off in zip(self.names, self.offs)}
        # device table of the staff-embedding gradient pointers: uploaded once, before the first kernel of the backward pass
        ptrs_host = torch.tensor([self.G[f"decoder.staff_emb.{w}_{sfx}"].data_ptr() for sfx in ("l0", "l0_reverse")
                                  for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")], dtype=torch.int64).pin_memory()
        self.G["__staff_emb_ptrs__"] = ptrs_host.to(dev, non_blocking=True)          # pinned: no stream synchronisation (the host keeps running ahead)
        self.keep_alive = [ptrs_host]
        self.dEnc = torch.zeros((B, T, H2), dtype=torch.float32, device=dev)
        self.dK = {p: torch.zeros((B, T, H), dtype=torch.float32, device=dev) for p in ("decoder", "decoder.upper_decoder", "decoder.lower_decoder")}
        # the two note decoders of a bar back-propagate concurrently on two side streams (see engine.side_streams); each accumulates its
        # encoder-output gradient in its own buffer (summed once at the end), everything else they write is per-staff already
        self.concurrent = bool(concurrent)
        self.dEnc_staff = [torch.zeros_like(self.dEnc), torch.zeros_like(self.dEnc)] if self.concurrent else [self.dEnc, self.dEnc]
        self.bar_major = bool(bar_major)
        # round 5: the note decoders' weight gradients run in finish(), on the weight-gradient stream beside the encoder's back-propagation
        # (eng.late_wgrads = False: where they were, behind each call's reverse loop on the staff's stream)
        lw = getattr(eng, "late_wgrads", None)
        self.late_wgrads = True if lw is None else bool(lw)
        self.late = []                                     # (closure, event on the issuing stream, tensors it reads): appended by any group's host thread
        self.clip_groups = list(clip_groups) if clip_groups else [(0, B)]
        self.d_hidden = torch.empty((B, H2), dtype=torch.float32, device=dev)       # gradient wrt the encoder's bridge output (initial bar-level hidden)
        self.group_flat = [self.flat] + [torch.zeros_like(self.flat) for _ in self.clip_groups[1:]]
        self.group_ptrs = [self.G["__staff_emb_ptrs__"]]
        for gf in self.group_flat[1:]:
            ph = (ptrs_host + (gf.data_ptr() - self.flat.data_ptr())).pin_memory()
            self.keep_alive.append(ph)
            self.group_ptrs.append(ph.to(dev, non_blocking=True))

    def decoder_group(self, gidx, gs, dts_g, dkey_g, dup_g, dlo_g):
        """Decoder backward of clip group gidx (gs: what Engine.forward saved for it) on the calling thread's current stream (+ the two
        side streams for group 0).  d*_g: gradients wrt the group's four output views (gs["outs"])."""
        from .engine import fork_on_streams, staff_streams, staves_concurrent
        eng, S, G, dev, T = self.eng, self.S, self.G, self.dev, self.T
        names, offs, group_flat, group_ptrs = self.names, self.offs, self.group_flat, self.group_ptrs
        dEnc, dK, dEnc_staff, d_hidden = self.dEnc, self.dK, self.dEnc_staff, self.d_hidden
        concurrent, bar_major = self.concurrent, self.bar_major
        L = hip.lib()
        cfg = eng.cfg
        H, Sz = cfg["hidden_size"], cfg["staff_emb_size"]
        te, ke, bars = cfg["time_sig_emb_size"], cfg["key_emb_size"], cfg["max_bars"]
        tokw = 4 * Sz + te + ke
        H2 = 2 * H
        b0, b1 = gs["range"]
        Bg = b1 - b0
        Gg = G if gidx == 0 else {k: group_flat[gidx][off:off + S[k].numel()].view(S[k].shape) for k, off in zip(names, offs)}
        Gg["__staff_emb_ptrs__"] = group_ptrs[gidx]
        enc_g, keys_g = gs["enc"], gs["keys"]
        if not enc_g.is_contiguous():
            raise ValueError("the group's slice of the encoder output is not contiguous: its range cannot be measured, and the decoder's products have no other arithmetic")
        enc_amax_g = hip.absmax(enc_g)      # max |enc| of the group's clips: the operand range of the decoder's deferred products (two-term fp16 split)
        dEnc_g = dEnc[b0:b1]
        dK_g = {p: t[b0:b1] for p, t in dK.items()}
        dEnc_staff_g = [t[b0:b1] for t in dEnc_staff]
        ts_out_g, key_out_g, up_out_g, lo_out_g = gs["outs"]
        # as in Engine.forward (engine.staff_streams); a group whose calls ran as persistent launches back-propagates its staves one after
        # the other (two persistent launches must never be in flight together)
        persist_g = any(seg["staff"][k][2].get("persist_ws") is not None for seg in gs["segments"] for k in ("up", "lo"))
        staves_g = staves_concurrent(gidx, len(self.clip_groups))
        seg_dh0 = {}                # segment index -> [dh0 of the upper call, dh0 of the lower call], rows = (bar in segment, clip)

        def segment_decoders_bwd(si_seg):
            """Both note decoders of a segment (bars decoded in one call each): they only need the loss gradients."""
            seg = gs["segments"][si_seg]
            bar0, nb = seg["bars"][0], len(seg["bars"])
            calls = []
            for si, (name, prefix, dout, out_t) in enumerate((("up", "decoder.upper_decoder", dup_g, up_out_g), ("lo", "decoder.lower_decoder", dlo_g, lo_out_g))):
                if bar_major:
                    maxs = out_t.shape[2]
                    dpr, pr = dout[bar0:bar0 + nb].view(nb * Bg, maxs, -1), out_t[bar0:bar0 + nb].view(nb * Bg, maxs, -1)
                else:
                    dpr, pr = dout[:, bar0], out_t[:, bar0]
                calls.append((eng, S, Gg, seg["staff"][name][2], keys_g[prefix], enc_g, dpr, pr, dK_g[prefix], dEnc_staff_g[si], Bg, T,
                              enc_amax_g, self.late if self.late_wgrads else None))
            issue = plan_staff_issue(concurrent, staves_g, persist_g, seg.get("pair") is not None, bool(L.a2s_debug_get(b"attn_pair")))
            if issue == "pair":
                # both staves' reverse loops from one host thread, their sweeps as one launch per step (as the forward ran them)
                streams = staff_streams(dev, gidx)
                (res,), events = fork_on_streams(dev, [streams[1]], [lambda: _note_decoder_bwd_pair(calls, streams, seg["pair"])])(wait=False)
                seg_dh0[si_seg] = (res, events)
            elif issue == "fork":    # one host thread per staff (engine.fork_on_streams); the current stream waits when the result is consumed
                seg_dh0[si_seg] = fork_on_streams(dev, staff_streams(dev, gidx), [lambda args=args: _note_decoder_bwd(*args) for args in calls])(wait=False)
            else:
                seg_dh0[si_seg] = ([_note_decoder_bwd(*args) for args in calls], [])

        # The note decoders' backward passes only need the loss gradients: all segments are enqueued up front (last segment first, as the
        # bar chain below consumes them), so the two staff streams run through every segment back to back instead of draining at each
        # segment boundary while the bar-level chain catches up.
        for si_seg in reversed(range(len(gs["segments"]))):
            segment_decoders_bwd(si_seg)

        bar_attn = []               # (q, ds, attention weights, dctx) of every bar: their key / encoder-output gradients in ONE call below
        d_hid_carry = None          # gradient wrt the bar-level hidden after bar k, coming from bar k+1
        d_token_next = None         # gradient wrt the (pre-dropout) token that bar k produced for bar k+1
        for bar in reversed(range(bars)):
            b = gs["bars"][bar]
            # ---- (1) the token this bar produced for the next one
            if d_token_next is not None:
                for rec in b["tok_rec"]:
                    _staff_token_bwd(eng, S, Gg, rec, d_token_next)
                ts_ids, key_ids, i64, stride = b["next_ids"]
                for table, ids_, col, width in (("decoder.time_sig_emb.weight", ts_ids, 4 * Sz, te), ("decoder.key_emb.weight", key_ids, 4 * Sz + te, ke)):
                    hip.check(L.a2s_embed_scatter_add(hip.stream(), hip._p(Gg[table]), hip._p(ids_) if i64 else None, None if i64 else hip._p(ids_), stride, 0,
                                                      hip._p(d_token_next), tokw, col, Bg, width, None, 1.0), "scatter ts/key")
            # ---- (2) heads: log_softmax + 3-layer MLP on headin = [bar_summary | ctx]
            d_headin = torch.zeros((Bg, 4 * H), dtype=torch.float32, device=dev)
            for hname, dout, out_t, nc in (("time_sig_out", dts_g, ts_out_g, cfg["num_time_sig"]), ("key_out", dkey_g, key_out_g, cfg["num_keys"])):
                t1, t2, lg, _ = b["heads"][hname]
                dlg = torch.empty((Bg, nc), dtype=torch.float32, device=dev)
                hip.check(L.a2s_log_softmax_bwd_rows(hip.stream(), _ptr(dout, bar * nc), _ptr(out_t, bar * nc), bars * nc, 1, hip._p(dlg), Bg, nc, Bg, 0),
                          "lsm bwd head")
                p = f"decoder.{hname}"
                dt2 = torch.empty_like(t2)
                _linear_bwd(t2, S[p + ".4.weight"], dlg, Gg, p + ".4.weight", p + ".4.bias", dx=dt2)
                hip.check(L.a2s_ew_act_bwd(hip.stream(), hip._p(dt2), hip._p(t2), hip._p(dt2), dt2.numel(), 1), "relu bwd")
                dt1 = torch.empty_like(t1)
                _linear_bwd(t1, S[p + ".2.weight"], dt2, Gg, p + ".2.weight", p + ".2.bias", dx=dt1)
                hip.check(L.a2s_ew_act_bwd(hip.stream(), hip._p(dt1), hip._p(t1), hip._p(dt1), dt1.numel(), 1), "relu bwd")
                _linear_bwd(b["headin"], S[p + ".0.weight"], dt1, Gg, p + ".0.weight", p + ".0.bias", dx=d_headin, dx_beta=1.0)
            # ---- (3) note decoders: both start from bar_summary
            d_hnew = torch.zeros((Bg, H2), dtype=torch.float32, device=dev)
            si_seg, j = b["seg"]
            dh0s, events = seg_dh0[si_seg]
            for ev in events:
                torch.cuda.current_stream().wait_event(ev)
            for dh0 in dh0s:
                d_hnew.add_(dh0[j * Bg:(j + 1) * Bg])
            d_hnew.add_(d_headin[:, :H2])
            if d_hid_carry is not None:
                d_hnew.add_(d_hid_carry)
            # ---- (4) bar-level GRU step + attention
            ldxb = tokw + H2
            dgi, dgh = torch.empty((Bg, 3 * H2), device=dev), torch.empty((Bg, 3 * H2), device=dev)
            dhp = torch.empty((Bg, H2), device=dev)
            hip.check(L.a2s_gru_gates_bwd(hip.stream(), hip._p(d_hnew), H2, None, 0, hip._p(b["gates"]), hip._p(b["hprev"]), H2, hip._p(dgi), 3 * H2, hip._p(dgh),
                                          3 * H2, None, 0, hip._p(dhp), H2, Bg, H2), "gates bwd bar")
            d_xbar = torch.empty((Bg, ldxb), device=dev)
            _linear_bwd(b["xbar"], S["decoder.gru.weight_ih_l0"], dgi, Gg, "decoder.gru.weight_ih_l0", "decoder.gru.bias_ih_l0", dx=d_xbar)
            _linear_bwd(b["hprev"], S["decoder.gru.weight_hh_l0"], dgh, Gg, "decoder.gru.weight_hh_l0", "decoder.gru.bias_hh_l0", dx=dhp, dx_beta=1.0)
            dq, ds = torch.empty((Bg, H), device=dev), torch.empty((1, Bg, T), device=dev)
            dctx = torch.empty((1, Bg, H2), device=dev)
            from .engine import bar_attn_workspace
            bar_ws = bar_attn_workspace(dev, gidx, Bg, T, H)
            if bar_ws is not None:
                # split-T kernels (round 5: 1.3 -> ~0.25 ms per bar at 248 clips): they load the saved context and its gradient 16 bytes at a time, so
                # the two odd-stride column blocks of the bar-level GRU input row are copied out first (0.5 MB each)
                ctx_c, dctx_c = b["xbar"][:, tokw:].contiguous(), d_xbar[:, tokw:].contiguous()
                hip.check(L.a2s_attn_step_bwd(hip.stream(), hip._p(keys_g["decoder"]), hip._p(enc_g), hip._p(b["qb"]), H, hip._p(S["decoder.attn.v.weight"]),
                                              hip._p(b["attw"]), hip._p(ctx_c), H2, hip._p(dctx_c), H2, _ptr(d_headin, H2), 4 * H, hip._p(dctx), H2, hip._p(dq), H,
                                              hip._p(ds), Bg, T, H, hip._p(bar_ws)), "attn bwd bar")
            else:
                hip.check(L.a2s_attn_step_bwd(hip.stream(), hip._p(keys_g["decoder"]), hip._p(enc_g), hip._p(b["qb"]), H, hip._p(S["decoder.attn.v.weight"]),
                                              hip._p(b["attw"]), _ptr(b["xbar"], tokw), ldxb, _ptr(d_xbar, tokw), ldxb, _ptr(d_headin, H2), 4 * H, hip._p(dctx), H2,
                                              hip._p(dq), H, hip._p(ds), Bg, T, H, None), "attn bwd bar")
            Wa = S["decoder.attn.attn.weight"]
            hip.gemm(dq, H, 1, Wa, 4 * H, 1, dhp, H2, Bg, H2, H, beta=1.0)                              # d hprev += dq W_h
            hip.gemm(dq, 1, H, b["hprev"], H2, 1, Gg["decoder.attn.attn.weight"], 4 * H, H, H2, Bg, beta=1.0)   # dW_h += dq^T hprev
            _colsum(dq, H, Gg["decoder.attn.attn.bias"], Bg, H)
            bar_attn.append((b["qb"].view(1, Bg, H), ds, b["attw"].view(1, Bg, T), dctx))
            d_hid_carry = dhp
            d_token = d_xbar[:, :tokw].contiguous()
            if b["keep"] is not None:
                d_token = d_token * b["keep"] / 0.9
            d_token_next = d_token
        # the bars' key / encoder-output gradients: one K = bars product per clip instead of `bars` rank-1 updates of the (T, 2H) gradient
        qs, dss, aws, dcs = [torch.cat(t, 0) for t in zip(*bar_attn)]
        _attn_deferred(eng, S, Gg, "decoder.attn", keys_g["decoder"], enc_g, qs, dss, aws, dcs, dK_g["decoder"], dEnc_g, Bg, T, H, len(bar_attn))
        # ---- initial token: <sos>/<eos> staff token (used for both staves) + time-signature / key <sos> rows
        d_sos = d_token_next.clone()
        d_sos[:, :2 * Sz] += d_sos[:, 2 * Sz:4 * Sz]
        _staff_token_bwd(eng, S, Gg, gs["sos_rec"][0], d_sos)
        for table, cid, col, width in (("decoder.time_sig_emb.weight", cfg["num_time_sig"], 4 * Sz, te), ("decoder.key_emb.weight", cfg["num_keys"], 4 * Sz + te, ke)):
            hip.check(L.a2s_embed_scatter_add(hip.stream(), hip._p(Gg[table]), None, None, 0, cid, hip._p(d_token_next), tokw, col, Bg, width, None, 1.0),
                      "scatter sos ts/key")
        d_hidden[b0:b1].copy_(d_hid_carry)
        return None


    def finish(self, grad_ready=None):
        eng, S, G, dev = self.eng, self.S, self.G, self.dev
        B, T, F = self.B, self.T, self.F
        names, offs, total, flat = self.names, self.offs, self.total, self.flat
        dEnc, dK = self.dEnc, self.dK
        sv = eng.saved
        assert sv["training"], "backward needs a forward run with training=True (batch statistics / saved activations)"
        L = hip.lib()
        H = eng.cfg["hidden_size"]
        H2 = 2 * H
        enc = sv["enc_out"]
        G["__staff_emb_ptrs__"] = self.group_ptrs[0]
        late_join = None
        if self.late:
            # The note decoders' weight gradients, on the weight-gradient stream: they start now (every closure waits for the event its call
            # recorded behind its reverse loop) and run beside the key products and the encoder's back-propagation below.  They accumulate
            # into their clip group's flat buffer; the groups' buffers are folded into `flat` on the same stream afterwards, over the decoder's
            # parameters only (nothing else is non-zero in them, and the main stream accumulates the encoder's gradients meanwhile), once the
            # key products below -- which write the other half of the decoders' attention matrices -- are done.
            dec_lo = next(off for k, off in zip(names, offs) if k.startswith("decoder."))
            assert all(k.startswith("decoder.") for k, off in zip(names, offs) if off >= dec_lo), "the decoder's parameters must be the tail of the flat layout"
            wg = _weight_grad_stream(dev)
            wg.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(wg):
                for fn, ev, tensors in self.late:
                    wg.wait_event(ev)
                    for t in tensors:
                        if t is not None:
                            t.record_stream(wg)
                    fn()
            late_join = dec_lo
            self.late = []
        else:
            for gf in self.group_flat[1:]:
                flat.add_(gf)
        d_hid_carry = self.d_hidden
        if self.concurrent:
            dEnc.add_(self.dEnc_staff[0]).add_(self.dEnc_staff[1])
        # ---- attention keys: K = enc W_e^T  ->  dW_e += dK^T enc ; dEnc += dK W_e
        enc2d = enc.view(B * T, H2)
        enc_amax = hip.absmax(enc)
        for p, dKp in dK.items():
            Wn = p + ".attn.attn.weight"
            dk_amax = hip.absmax(dKp)
            # (tall-K kernel: dK packed, enc streamed once, the result into columns 2H.. of the 4H-wide matrix; csrc/a2s_linear.hip)
            if not hip.tallk_wgrad(dKp, 0, H, enc2d, 0, H2, G[Wn], H2, 4 * H, B * T, H, H2, dk_amax, enc_amax):
                sk = L.a2s_gemm_pick_splitk(H, H2, B * T, 1)
                hip.gemm(dKp, 1, H, enc2d, H2, 1, G[Wn], 4 * H, H, H2, B * T, beta=1.0, splitk=sk, c_off=H2, two_term=(dk_amax, enc_amax))
            hip.gemm(dKp, H, 1, S[Wn], 4 * H, 1, dEnc, H2, B * T, H2, H, beta=1.0, b_off=H2, two_term=(dk_amax, hip.absmax(S[Wn])))
        if late_join is not None:
            wg = _weight_grad_stream(dev)
            wg.wait_stream(torch.cuda.current_stream())            # (the key products above)
            with torch.cuda.stream(wg):
                for gf in self.group_flat[1:]:
                    flat[late_join:].add_(gf[late_join:])
                if Backward.check_fold:                      # tests: nothing but decoder gradients may sit in the groups' own buffers
                    for gi, gf in enumerate(self.group_flat[1:], 1):
                        assert not bool(gf[:late_join].any()), f"clip group {gi}: non-decoder gradients in the group buffer would be lost by the late fold"
        # The encoder's last weight gradients (layer 0: ~5 ms of GEMMs on the weight-gradient stream, nothing of the encoder left to run beside
        # them) overlap with the START of the ConvStack backward: the caller's stream does not wait for them here.  The decoder + encoder slice
        # is announced from that stream (a collective issued there is ordered behind its work, which itself waited for everything the main
        # stream had enqueued when those GEMMs were launched), and the main stream joins it after the ConvStack backward.
        d_conv = _encoder_bwd(eng, S, G, sv["enc"], dEnc, d_hid_carry, B, T)
        n_conv = next(off for k, off in zip(names, offs) if not k.startswith("convstack."))      # state_dict order: convstack first
        if grad_ready is not None:
            with torch.cuda.stream(_weight_grad_stream(dev)):
                grad_ready(self.flat_full, n_conv, total + 1)           # (+ the loss word)
        if getattr(eng, "conv_unperm", None) is not None:       # the ConvStack ran before the clips were permuted into their groups (train.TrainStep)
            d_conv = d_conv.reshape(B, T, -1).index_select(0, eng.conv_unperm)
        _convstack_bwd(eng, S, G, sv["conv"], d_conv, B, T, F)
        torch.cuda.current_stream().wait_stream(_weight_grad_stream(dev))
        if grad_ready is not None:
            grad_ready(flat, 0, n_conv)
        G[None] = flat
        G["__loss_gate__"] = self.flat_full[total:]
        eng._keep_alive = self.keep_alive
        return G




def backward(eng, S, grad_outputs, grad_ready=None, loss_total=None):
    """Gradients of sum_i <out_i, grad_outputs_i> wrt every parameter.  Returns dict name -> tensor (views of ONE flat buffer,
    also returned as `flat` under key None) in state_dict parameter order.
    grad_ready(flat, start, end): optional callback, called when flat[start:end] is final (everything that writes it has been
    enqueued on the current stream) -- first the encoder + decoder slice, then the ConvStack slice; train.GradientExchange starts
    the data-parallel all-reduce of a slice there, under the rest of the backward pass."""
    from .engine import group_views, run_clip_groups
    sv = eng.saved
    assert sv["training"], "backward needs a forward run with training=True (batch statistics / saved activations)"
    dev = sv["enc_out"].device
    clip_groups = sv.get("clip_groups") or [(0, sv["shape"][0])]
    ctx = Backward(eng, S, sv["shape"], dev, clip_groups, sv.get("concurrent"), sv.get("bar_major"))
    dts, dkey, dup, dlo = [g.contiguous() for g in grad_outputs]

    def group(gidx):
        b0, b1 = clip_groups[gidx]
        if ctx.bar_major:
            dup_g, dlo_g = group_views(dup, clip_groups, gidx), group_views(dlo, clip_groups, gidx)
        else:
            dup_g, dlo_g = dup[b0:b1], dlo[b0:b1]
        ctx.decoder_group(gidx, sv["groups"][gidx], dts[b0:b1], dkey[b0:b1], dup_g, dlo_g)

    run_clip_groups(dev, [lambda gi=gi: group(gi) for gi in range(len(clip_groups))])
    if loss_total is not None:
        ctx.flat_full[ctx.total:].copy_(loss_total.reshape(1))
    return ctx.finish(grad_ready)


def _weight_grad_stream(dev):
    from .engine import group_stream
    return group_stream(dev, 1)             # the fourth stream of the budget: idle while the encoder back-propagates


def _encoder_bwd(eng, S, G, es, dEnc, d_hidden, B, T):
    """The caller's stream is NOT made to wait for the weight gradients on _weight_grad_stream(dev) (layer 0's run after its recurrence, with
    nothing left to hide them under): the caller waits for that stream before anything reads the encoder's gradient slice (Backward.finish
    announces the slice FROM that stream and joins it after the ConvStack backward)."""
    L = hip.lib()
    H = eng.cfg["hidden_size"]
    dev = dEnc.device
    W = S["encoder.fc.weight"]
    # bridge: hidden = tanh(pre); pre_l = fc([hf_l ; hr_l])
    dpre = torch.empty_like(d_hidden)
    hip.check(L.a2s_ew_act_bwd(hip.stream(), hip._p(d_hidden), hip._p(es["hidden"]), hip._p(dpre), dpre.numel(), 2), "tanh bwd")
    dhn = []
    for l in (0, 1):
        for half, hfin in enumerate((es["finals"][2 * l], es["finals"][2 * l + 1])):
            d = torch.empty((B, H), device=dev)
            hip.gemm(dpre, 2 * H, 1, W, 2 * H, 1, d, H, B, H, H, a_off=l * H, b_off=half * H)                       # d h_fin = dpre_l W[:, half]
            hip.gemm(dpre, 1, 2 * H, hfin, H, 1, G["encoder.fc.weight"], 2 * H, H, H, B, beta=1.0, a_off=l * H, c_off=half * H)   # dW += dpre_l^T h_fin
            dhn.append(d)
        _colsum(dpre, 2 * H, G["encoder.fc.bias"], B, H, x_off=l * H)
    gws = [hip.gru_workspace(B, H, dev), hip.gru_workspace(B, H, dev)]
    in_amax = hip.absmax(es["layers"][0]["in"])        # max of the ConvStack features (layer 0's input)
    dout = dEnc                                              # gradient wrt layer-1 outputs (B,T,2H)
    for layer in (1, 0):
        ls = es["layers"][layer]
        inp = ls["in"]                                       # (B*T, I)
        I = inp.shape[1]
        out = ls["out"]
        dX = torch.empty((B * T, I), device=dev)
        from .engine import encoder_streams, fork_on_streams
        streams = encoder_streams(dev, B)                 # the two directions' BPTT chains are independent: one stream (and host thread) each

        def direction(d, sfx):
            dgi = torch.empty((B, T, 3 * H), device=dev)
            dghs = torch.empty((B, T, 3 * H), device=dev)
            dgh_first, dhbuf, dgh_tmp = torch.empty((B, 3 * H), device=dev), torch.empty((2, B, H), device=dev), torch.empty((B, 3 * H), device=dev)
            # max |dgi|, max |dghs| (the operand ranges of dX and of the deferred weight gradients) come out of the persistent BPTT launch, which
            # holds every element in a register; the launch-per-step kernels do not produce them (valid = 0): the tensors are measured then
            ranges, valid = torch.empty(2, device=dev), C.c_int(0)
            if L.a2s_debug_get(b"tallk_wgrad") > 0:
                hip.check(L.a2s_gru_seq_bwd_ranged(hip.stream(), _ptr(dout, d * H), T * 2 * H, 2 * H, _ptr(out, d * H), T * 2 * H, 2 * H, hip._p(ls["dirs"][d]["gates"]),
                                                   hip._p(S[f"encoder.gru.weight_hh_{sfx}"]), hip._p(dhn[2 * layer + d]), hip._p(dgi), hip._p(dghs), hip._p(dgh_first),
                                                   hip._p(dhbuf), hip._p(dgh_tmp), B, T, H, d, hip._p(gws[d]), gws[d].numel() * 4, hip._p(ranges), C.byref(valid)),
                          "a2s_gru_seq_bwd_ranged")
            else:
                hip.check(L.a2s_gru_seq_bwd(hip.stream(), _ptr(dout, d * H), T * 2 * H, 2 * H, _ptr(out, d * H), T * 2 * H, 2 * H, hip._p(ls["dirs"][d]["gates"]),
                                            hip._p(S[f"encoder.gru.weight_hh_{sfx}"]), hip._p(dhn[2 * layer + d]), hip._p(dgi), hip._p(dghs), hip._p(dgh_first),
                                            hip._p(dhbuf), hip._p(dgh_tmp), B, T, H, d, hip._p(gws[d]), gws[d].numel() * 4), "a2s_gru_seq_bwd")
            return (dgi, dghs, dgh_first, dhbuf, dgh_tmp, ranges if valid.value else None)

        res = fork_on_streams(dev, streams, [lambda d=d, sfx=sfx: direction(d, sfx) for d, sfx in enumerate((f"l{layer}", f"l{layer}_reverse"))])()
        dgi_amax = []
        # input gradient (what the next recurrence / the ConvStack needs) on the current stream ...
        for d, sfx in enumerate((f"l{layer}", f"l{layer}_reverse")):
            dgi2 = res[d][0].view(B * T, 3 * H)
            Wih = S[f"encoder.gru.weight_ih_{sfx}"]
            ranges = res[d][5]
            tt = (ranges[0:1] if ranges is not None else hip.absmax(dgi2), hip.absmax(Wih))        # ranges: the two-term fp16 split
            dgi_amax.append(tt[0])
            if L.a2s_debug_get(b"gemm_bf16x3") > 0:      # k-contiguous weight copy (<= 1.5 MB): both operands on the GEMM's split-operand path
                hip.gemm(dgi2, 3 * H, 1, Wih.t().contiguous(), 1, 3 * H, dX, I, B * T, I, 3 * H, beta=0.0 if d == 0 else 1.0, two_term=tt)
            else:
                hip.gemm(dgi2, 3 * H, 1, Wih, I, 1, dX, I, B * T, I, 3 * H, beta=0.0 if d == 0 else 1.0, two_term=tt)
        # ... the weight gradients (MFMA-bound, nobody waits for them) on a third stream, under the next layer's latency-bound recurrence
        wg = _weight_grad_stream(dev)
        ev = torch.cuda.Event()
        ev.record()
        wg.wait_event(ev)
        for d, sfx in enumerate((f"l{layer}", f"l{layer}_reverse")):
            dgi, dghs, dgh_first, ranges = res[d][0], res[d][1], res[d][2], res[d][5]
            # (everything the weight-gradient stream reads that was allocated on another stream -- the operand-range scalars included: freed by
            # this function's return, their blocks would be handed to the next small allocation of the main stream while these GEMMs still run)
            for t in (dgi, dghs, dgh_first, dgi_amax[d], in_amax, ranges):
                if t is not None:
                    t.record_stream(wg)
            with torch.cuda.stream(wg):
                dgi2, dghs2 = dgi.view(B * T, 3 * H), dghs.view(B * T, 3 * H)
                # Tall-K kernel (csrc/a2s_linear.hip): the GRADIENT is the streamed operand -- read once, its column sums (the bias gradient) taken
                # on the way -- the layer's input / output is packed, and the result lands transposed, in the parameter's (3H, I) layout.
                x_bound = in_amax if layer == 0 else hip.one(dev)
                if not hip.tallk_wgrad(inp, 0, I, dgi2, 0, 3 * H, G[f"encoder.gru.weight_ih_{sfx}"], 0, I, B * T, I, 3 * H, x_bound, dgi_amax[d],
                                       transposed=True, bias=G[f"encoder.gru.bias_ih_{sfx}"]):
                    _linear_bwd(inp, S[f"encoder.gru.weight_ih_{sfx}"], dgi2, G, f"encoder.gru.weight_ih_{sfx}", f"encoder.gru.bias_ih_{sfx}",
                                dy_amax=dgi_amax[d], x_bound=x_bound)
                dghs_amax = ranges[1:2] if ranges is not None else hip.absmax(dghs2)
                if not hip.tallk_wgrad(out, d * H, 2 * H, dghs2, 0, 3 * H, G[f"encoder.gru.weight_hh_{sfx}"], 0, H, B * T, H, 3 * H,
                                       hip.one(dev), dghs_amax, transposed=True, bias=G[f"encoder.gru.bias_hh_{sfx}"]):
                    sk = L.a2s_gemm_pick_splitk(3 * H, H, B * T, 1)
                    hip.gemm(dghs2, 1, 3 * H, out, 2 * H, 1, G[f"encoder.gru.weight_hh_{sfx}"], H, 3 * H, H, B * T, beta=1.0, splitk=sk, b_off=d * H,
                             two_term=(dghs_amax, hip.one(dev)))
                    _colsum(dghs2, 3 * H, G[f"encoder.gru.bias_hh_{sfx}"], B * T, 3 * H)
                _colsum(dgh_first, 3 * H, G[f"encoder.gru.bias_hh_{sfx}"], B, 3 * H)
        dout = dX.view(B, T, I)
    return dout                                              # (B, T, conv_feature_size)


# How the ConvStack's backward is laid out: conv_bwd_plan.ConvBwdFlags describes each switch.  Module attributes (tests and tools assign them; _convstack_bwd
# reads them once per call); the one environment switch is the documented fallback A2S_FUSE_BN_ROWS=0.
_FUSE_BN_APPLY = False
_FUSE_BN_APPLY_L1 = True
_DGRAD_BNSTATS = True
_SYNC_FUSED = True
_LIN_WGRAD_AT = "before"
_FUSE_BN_ROWS = os.environ.get("A2S_FUSE_BN_ROWS", "1") != "0"
# the gradient entering a layer with what the kernel that wrote it reduced on the way: statistics partials (tensor, blocks), max |g| (scalar or per channel)
GradIn = namedtuple("GradIn", "g partial amax", defaults=(None, None))


def _bn_bwd(source, eng, G, name, gin, x, bn, dims, mask=None, dx=None, amax=None):
    """BatchNorm backward of gin.g, statistics from `source` (conv_bwd_plan.stats_source); dx None: statistics only.  Returns c12, the per-channel means."""
    dgamma, dbeta = G[name + ".weight"], G[name + ".bias"]
    if source in ("own", "partial"):
        return hip.bn_bwd(gin.g, x, bn, mask, dgamma, dbeta, dx, dims, amax, gin.partial if source == "partial" else None)
    import torch.distributed as dist          # statistics of the global minibatch (see Engine.__init__)
    return hip.bn_bwd_sync(gin.g, x, bn, mask, dgamma, dbeta, dims, eng.bn_counts[name], dist.all_reduce, gin.partial if source == "sync_partial" else None)


def _convstack_bwd(eng, S, G, cs, d_out, B, T, F):
    """Walks conv_bwd_plan.plan_convstack_bwd: every decision is the plan's, this function allocates and launches."""
    if cs["a4"] is not None:
        raise ValueError("the Linear's input is re-formed from y4 on the fly: a materialised a4 has no backward path")
    L, dev, Cf, rows = hip.lib(), d_out.device, eng.cfg["conv_feature_size"], B * T
    flags = ConvBwdFlags(_FUSE_BN_ROWS, _DGRAD_BNSTATS, _SYNC_FUSED, _FUSE_BN_APPLY, _FUSE_BN_APPLY_L1, _LIN_WGRAD_AT)
    lin, layers = plan_convstack_bwd(flags, eng.sync_bn, rows, F, hip.LINEAR_KERNELS, bool(L.a2s_linear_dgrad_eligible(rows, 40 * F, Cf, F)),
                                     {c: bool(L.a2s_conv3x3_wgrad_bn_ranged_eligible(F, *c)) for c in CHANS[1:]})
    scalar = lambda: torch.zeros(1, dtype=torch.float32, device=dev)
    # dropout + ReLU + BatchNorm1d over the (B*T, Cf) Linear output, in place
    dz, dz_amax = d_out.reshape(rows, Cf).contiguous(), scalar()
    _bn_bwd(lin.stats, eng, G, "convstack.out_bn", GradIn(dz), cs["z"], cs["out_bn"], (rows, Cf, 1), cs["drop"], dz, dz_amax)
    if lin.absmax_after:
        hip.absmax(dz, dz_amax)
    # Linear 19200 -> Cf, no bias, which read relu(bn4(y4)) on the fly (so does its weight gradient):  dW += dz^T a4 ; da4 = dz W
    Wout, y4, bn4 = S["convstack.out.weight"], cs["y"][3].view(rows, 40 * F), cs["bn"][3]
    da = torch.empty_like(y4)

    def lin_wgrad():
        if not hip.linear_wgrad(dz, y4, (bn4[2], bn4[3], F), dz_amax, cs["abound"][3], G["convstack.out.weight"]):       # csrc/a2s_linear.hip
            _linear_bwd(y4, Wout, dz, G, "convstack.out.weight", None, x_affine=(bn4[2], bn4[3], F), dy_amax=dz_amax, x_bound=cs["abound"][3])
    def lin_wgrad_beside():          # on the weight-gradient stream, after everything the main stream holds so far
        wg_stream, ev = _weight_grad_stream(dev), torch.cuda.Event()
        ev.record()
        wg_stream.wait_event(ev)
        with torch.cuda.stream(wg_stream):
            lin_wgrad()
    if lin.wgrad_at in ("before", "beside"):
        (lin_wgrad if lin.wgrad_at == "before" else lin_wgrad_beside)()
    gin = GradIn(da.view(B, T, 40, F))
    if lin.dgrad == "gemm":
        hip.gemm(dz, Cf, 1, Wout, 40 * F, 1, da, 40 * F, rows, 40 * F, Cf)
    else:
        w_amax = cs["w_out_amax"] if cs.get("w_out_amax") is not None else hip.absmax(Wout)
        gin = GradIn(gin.g, *hip.linear_dgrad_bnstats(dz, Wout, da, y4, bn4, F, dz_amax, w_amax, lin.dgrad == "own"))
    for lp in layers:
        i, ci, co, g = lp.i, lp.ci, lp.co, gin.g
        y, bn_i, dW = cs["y"][i - 1], cs["bn"][i - 1], G[f"convstack.conv{i}.weight"]          # pre-BN conv output of this layer, ...
        x_in, in_bn, in_bound = (cs["y"][i - 2], cs["bn"][i - 2], cs["abound"][i - 2]) if i > 1 else (cs["x0"], None, None)
        ws = torch.empty(L.a2s_conv3x3_wgrad_workspace_bytes(ci, co) // 4, dtype=torch.float32, device=dev)
        dy_amax = scalar() if lp.dy_range else None          # max |dy|: the two-term fp16 kernels scale their operand by the matching power of two
        if lp.lin_wgrad:
            lin_wgrad_beside()
        bn_args = (lp.stats, eng, G, f"convstack.bn{i}", gin, y, bn_i, (rows, co, F))
        dy = g                                                 # in place, but for "tiled"
        if lp.form == "rows":
            hip.conv3x3_wgrad_bn(g, y, bn_i, _bn_bwd(*bn_args), None, x_in, in_bn, dW, ws, ranged=(gin.amax, cs["yabs"][i - 1], dy_amax, in_bound))
        elif lp.form == "apply":
            _bn_bwd(*bn_args, dx=g, amax=dy_amax)
            if lp.absmax_after:            # (the synchronised apply pass does not reduce the range of what it writes)
                hip.absmax(g, dy_amax)
            hip.conv3x3_wgrad(g, x_in.view(B, T, ci, F), in_bn[2] if in_bn else None, in_bn[3] if in_bn else None, dW, ws, dy_amax, in_bound)
        else:
            dy = torch.empty_like(g) if i > 1 else None
            hip.conv3x3_wgrad_bn(g, y, bn_i, _bn_bwd(*bn_args), dy, x_in, in_bn, dW, ws)
        if lp.dgrad == "none":
            break
        gprev, cws = torch.empty((B, T, ci, F), dtype=torch.float32, device=dev), hip.conv_workspace(co, dev)
        below = nblk = out_amax = None
        if lp.dgrad == "bnstats":                              # statistics partials of the layer below, and its per-channel range, from the epilogue
            nblk = L.a2s_conv3x3_stat_blocks(B, T, F, co)
            below = (x_in, in_bn, torch.empty((nblk, ci, 2), dtype=torch.float32, device=dev))
            out_amax = torch.empty(ci, dtype=torch.float32, device=dev) if lp.out_range else None      # max |g| per channel (zeroed by the launch)
        hip.conv3x3_dgrad(dy, S[f"convstack.conv{i}.weight"], gprev, cws, below, dy_amax if lp.dgrad_range else None, out_amax)
        gin = GradIn(gprev, (below[2], nblk) if below else None, out_amax)
    if lin.join_side:
        torch.cuda.current_stream().wait_stream(_weight_grad_stream(dev))      # the Linear's weight gradient, issued beside the chain above
