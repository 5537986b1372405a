"""TEST INFRASTRUCTURE ONLY.  One NoteDecoder.decode_notes call (a2s_note_decoder_fwd / a2s_note_decoder_bwd, include/a2s.h) restated in plain torch
on the CPU, in float64 or float32: what tests/test_gpu_note_decoder_call.py holds every path of the call to, tensor by tensor, step by step, row by row.

Built on oracle/model_ref.py's `attention` and `gru_cell` with a step loop of its own, because the call does what model_ref.decode_notes cannot:
  * rows = bars x clips (row = bar * n_clips + clip): the rows of a clip share its encoder outputs and its key projection;
  * per-step teacher-forcing bit masks: bit g of flags[t] teacher-forces bar g at step t, every other row feeds back its own argmax (torch.argmax: the
    lowest index on ties);
  * the key projection is a LEAF: K = enc W_e^T is formed once and detached; the encoder outputs themselves enter only the context product.  The
    leaf gradients are then exactly what the call accumulates into its dK and dEnc arguments (engine_bwd.Backward.finish turns dK into the key half of
    attn.attn.weight's gradient and the rest of dEnc afterwards: "attention keys: K = enc W_e^T -> dW_e += dK^T enc"), and the gradient this file
    returns for attn.attn.weight is non-zero in its query half (columns [:, :2H]) only;
  * `until`: rows are independent here, so a row simply keeps running; the caller zeroes dprobs at t >= until[row] and compares at t < until[row].  A
    row that runs on behind `until` then contributes nothing -- the contract of "finished rows" in include/a2s.h.

The attention is model_ref.attention itself, fed the query q = h W_h^T + b in the place of the state, the key rows in the place of the encoder
outputs and [I | I] as its Linear: cat(q, K) [I | I]^T = q + K, exactly (products with 1 and 0, sums with 0), in either precision.

Imports nothing of the product package but the token constants."""
import torch
import torch.nn.functional as F

from oracle.model_ref import attention, gru_cell
from piano_a2s_amd.spec import EOS, SOS

# the ten tensors of a note decoder, by the reference's state_dict names behind the decoder's prefix
SUFFIXES = (".attn.attn.weight", ".attn.attn.bias", ".attn.v.weight", ".gru.weight_ih_l0", ".gru.weight_hh_l0", ".gru.bias_ih_l0", ".gru.bias_hh_l0",
            ".out.weight", ".out.bias", ".embedding.weight")


def prefix_tensors(state, prefix):
    """The ten decoder tensors of `prefix` out of a state dict, keyed by SUFFIXES."""
    return {s: state[prefix + s] for s in SUFFIXES}


def forced_rows(flag, groups, n_clips):
    """(rows,) bool: the rows whose bar the step's flag teacher-forces."""
    bar = torch.arange(groups * n_clips) // n_clips
    return ((int(flag) >> bar) & 1).bool()


def decode_call(W, enc, h0, gt, flags, groups, n_clips, steps, max_steps, dtype=torch.float64, grad=False):
    """One call over rows = groups * n_clips.  W: SUFFIXES -> tensor; enc (n_clips, T, 2H); h0 (rows, 2H); gt (rows, >= steps) int64 or None (greedy:
    every row feeds back, the loop ends once every row has emitted <eos>, as models.py:388-419); flags: per step, bit g = bar g is teacher-forced.
    Returns a dict: per-step tensors in the layouts the library saves (h (n+1, R, 2H); x (n+1, R, E+2H) = [token | ctx], slot n holding only the
    next token; q (n, R, H); o (n, R, 4H) = [h' | ctx]; gates (n, R, 8H) = [r | z | n | gh_n]; attw (n, R, T)), probs (R, n, V) log-probabilities,
    ids (R, n) their argmax, fed (R, n) the token each step handed on, lengths (R,), steps = n executed, margin (R, n) top-2 log-probability gap of
    every decision and fed_back (R, n) bool: the decisions that were fed back AND consumed by a later executed step.  With grad=True the tensors
    keep their graph and `leaves` holds what `call_backward` differentiates with respect to."""
    R, H2 = h0.shape
    H = H2 // 2
    assert R == groups * n_clips and enc.shape[0] == n_clips and enc.shape[2] == H2
    P = {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in W.items()}
    enc_l = enc.detach().to(dtype).clone().requires_grad_(grad)
    h0_l = h0.detach().to(dtype).clone().requires_grad_(grad)
    Wa, ba, emb = P[".attn.attn.weight"], P[".attn.attn.bias"], P[".embedding.weight"]
    K = (enc_l.detach() @ Wa.detach()[:, H2:].t()).requires_grad_(grad)          # (n_clips, T, H): the leaf
    clip = torch.arange(R) % n_clips
    K_rows, enc_rows = K[clip], enc_l[clip]
    eye = torch.eye(H, dtype=dtype)
    PA = {"a.attn.weight": torch.cat([eye, eye], dim=1), "a.attn.bias": torch.zeros(H, dtype=dtype), "a.v.weight": P[".attn.v.weight"]}
    w_ih, w_hh, b_ih, b_hh = (P[".gru." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
    greedy = gt is None
    h = h0_l
    tok = F.embedding(torch.full((R,), SOS, dtype=torch.long), emb)
    hs, xs, qs, os_, gs, aws, lps, ids, fed, margins, fb = [h], [], [], [], [], [], [], [], [], [], []
    eos_seen = torch.zeros(R, dtype=torch.bool)
    lengths = torch.full((R,), max_steps, dtype=torch.long)
    n = 0
    for t in range(steps):
        if greedy and bool(eos_seen.all()):
            break
        q = h @ Wa[:, :H2].t() + ba
        a = attention(q.unsqueeze(0), K_rows, PA, "a")                           # (R, T) = softmax_T(v . tanh(q + K))
        ctx = torch.bmm(a.unsqueeze(1), enc_rows).squeeze(1)
        x = torch.cat([tok, ctx], dim=1)
        hn = gru_cell(x, h, w_ih, w_hh, b_ih, b_hh)
        # the gates the library saves, by the same formulas (test_note_decoder_oracle_cpu.py rebuilds h from them)
        gi, gh = x @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :H2] + gh[:, :H2])
        z = torch.sigmoid(gi[:, H2:2 * H2] + gh[:, H2:2 * H2])
        ng = torch.tanh(gi[:, 2 * H2:] + r * gh[:, 2 * H2:])
        o = torch.cat([hn, ctx], dim=1)
        lp = F.log_softmax(o @ P[".out.weight"].t() + P[".out.bias"], dim=-1)
        am = torch.argmax(lp, dim=-1)
        top = lp.detach().topk(2, dim=-1)[0]
        forced = torch.zeros(R, dtype=torch.bool) if greedy else forced_rows(flags[t], groups, n_clips)
        nxt = am if greedy else torch.where(forced, gt[:, t], am)
        hit = (am == EOS) if greedy else (gt[:, t] == EOS)
        eos_seen |= hit
        lengths = torch.where(hit, torch.full_like(lengths, t + 1), lengths)
        tok = F.embedding(nxt, emb)
        h = hn
        n = t + 1
        hs.append(h); xs.append(x); qs.append(q); os_.append(o); gs.append(torch.cat([r, z, ng, gh[:, 2 * H2:]], dim=1)); aws.append(a); lps.append(lp)
        ids.append(am); fed.append(nxt); margins.append(top[:, 0] - top[:, 1]); fb.append(~forced)
    xs.append(torch.cat([tok, torch.zeros(R, H2, dtype=dtype)], dim=1))
    fed_back = torch.stack(fb, dim=1)
    fed_back[:, n - 1] = False                      # (nothing consumes what the last executed step hands on)
    st = lambda ts: torch.stack(ts, dim=0)
    return dict(h=st(hs), x=st(xs), q=st(qs), o=st(os_), gates=st(gs), attw=st(aws), probs=torch.stack(lps, dim=1), ids=torch.stack(ids, dim=1),
                fed=torch.stack(fed, dim=1), lengths=lengths, steps=n, margin=torch.stack(margins, dim=1), fed_back=fed_back,
                leaves=dict(P=P, enc=enc_l, h0=h0_l, K=K))


def live_pairs(until, rows, n):
    """(rows, n) bool: the (row, step) pairs that still ran, t < until[row]; every pair without `until`."""
    if until is None:
        return torch.ones(rows, n, dtype=torch.bool)
    return torch.arange(n).unsqueeze(0) < until.to(torch.long).unsqueeze(1)


def call_backward(fwd, dprobs, until=None):
    """Reverse of decode_call(grad=True) under dprobs (R, n, V), zeroed wherever t >= until[row].  Returns dict(dh0 (R, 2H), dK (n_clips, T, H),
    dEnc (n_clips, T, 2H), params: SUFFIXES -> gradient; attn.attn.weight's is zero in its key half, see the module docstring)."""
    probs = fwd["probs"]
    R, n, _ = probs.shape
    d = dprobs.detach().to(probs.dtype) * live_pairs(until, R, n).unsqueeze(2).to(probs.dtype)
    lv = fwd["leaves"]
    for t in [lv["enc"], lv["h0"], lv["K"], *lv["P"].values()]:
        t.grad = None
    torch.autograd.backward(probs, d)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(dh0=zero(lv["h0"]), dK=zero(lv["K"]), dEnc=zero(lv["enc"]), params={k: zero(v) for k, v in lv["P"].items()})


FWD_TENSORS = ("h", "x", "q", "o", "gates", "attw", "probs")


def reference(W, enc, h0, gt, flags, groups, n_clips, steps, max_steps, until=None, dprobs=None):
    """The float64 run and what the float32 run of the same code loses against it: returns (f64 forward dict, f64 gradients or None, dev) with
    dev[name] = max |f32 - f64| / max |f64| per tensor of FWD_TENSORS over the live pairs (x split into "x_emb" / "x_ctx", h without slot 0) and, with
    dprobs, per gradient ("dh0", "dK", "dEnc", SUFFIXES).  Both runs must take the same decisions (asserted): the inputs' argmax margins see to that."""
    runs = {}
    for dt in (torch.float64, torch.float32):
        f = decode_call(W, enc, h0, gt, flags, groups, n_clips, steps, max_steps, dtype=dt, grad=dprobs is not None)
        g = call_backward(f, dprobs, until) if dprobs is not None else None
        runs[dt] = ({k: (v.detach() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in f.items() if k != "leaves"}, g)
    (f64, g64), (f32, g32) = runs[torch.float64], runs[torch.float32]
    assert f64["steps"] == f32["steps"] and torch.equal(f64["ids"], f32["ids"]), "the float32 run of the oracle left the float64 run's path: a near-tie in the inputs"
    E = W[".embedding.weight"].shape[1]
    live = live_pairs(until, h0.shape[0], f64["steps"])
    dev = {}
    for name, a, b in forward_views(f64, f32, E):
        dev[name] = rel_err(b, a, live)
    if g64 is not None:
        for name, a, b in grad_views(g64, g32):
            dev[name] = rel_err(b, a, None)
    return f64, g64, dev


def forward_views(ref, got, E):
    """(name, ref, got) of every forward tensor as (rows, steps, width): what a comparison at the live (row, step) pairs walks."""
    n = ref["steps"]
    rs = lambda t: t[:n].transpose(0, 1)
    out = [("h", rs(ref["h"][1:]), rs(got["h"][1:])), ("x_emb", rs(ref["x"])[:, :, :E], rs(got["x"])[:, :, :E]), ("x_ctx", rs(ref["x"])[:, :, E:], rs(got["x"])[:, :, E:])]
    out += [(k, rs(ref[k]), rs(got[k])) for k in ("q", "o", "gates", "attw")]
    out.append(("probs", ref["probs"][:, :n], got["probs"][:, :n]))
    return out


def grad_views(ref, got):
    out = [(k, ref[k], got[k]) for k in ("dh0", "dK", "dEnc")]
    return out + [(k, ref["params"][k], got["params"][k]) for k in SUFFIXES]


def rel_err(got, ref, live=None):
    """max |got - ref| over max |ref|, both over the live (row, step) pairs when `live` (rows, steps) is given (tensors (rows, steps, width))."""
    d = (got.double() - ref.double()).abs()
    m = ref.double().abs()
    if live is not None:
        d, m = d[live], m[live]
    return float(d.max()) / max(float(m.max()), 1e-300) if d.numel() else 0.0


def worst(got, ref, live=None):
    """Index (as a tuple) and size of the largest |got - ref|, live pairs only: tells the author WHICH row and step are wrong."""
    d = (got.double() - ref.double()).abs()
    d = torch.nan_to_num(d, nan=float("inf"))
    if live is not None:
        d = torch.where(live.unsqueeze(2), d, torch.zeros_like(d))
    i = int(d.argmax())
    idx = []
    for s in reversed(d.shape):
        idx.append(i % s)
        i //= s
    return tuple(reversed(idx)), float(d.max())
