"""TEST INFRASTRUCTURE: the CPU oracle's decode loops with the token choice as a parameter, recording every attention row.

Composes the parts of `oracle.model_ref` (convstack_forward, encoder_forward, attention, gru_cell, _staff_token) into the reference's two loops,
operation for operation, as tests/constrained_oracle.py does.  The token choice is delegated:
  * `PlainChoice()`            -- argmax of the log-probabilities: `oracle.model_ref.forward(..., inference=True)`;
  * `GrammarChoice(grammar)`   -- the constrained choice of tests/constrained_oracle.py;
  * ground truth given         -- `oracle.model_ref.forward(..., inference=False, ground_truth=gt, teacher_forcing_ratio=1.0)`: every note step and every
                                  bar consumes the given ids, the <eos> bookkeeping follows them (the forced alignment of a known score).
(tests/test_align_oracle_cpu.py asserts `torch.equal` on all four outputs for the first and the last: that validates the helper.)

Every `model_ref.attention` row is kept.  Next to the four outputs the helper returns, per attention layer ("bar", "up", "lo"), the float64 summaries
    peak (lowest index of the row's maximum), weight (the row's value there), centroid (sum_t t * a[t])
with the fills of the device arrays where no step ran (peak -1, weight 0, centroid -1), and the full float32 weights (zeros where no step ran)."""
import torch
import torch.nn.functional as F

from oracle import model_ref
from oracle.model_ref import EOS, PAD, SOS, VOCAB_SIZE
from tests.constrained_oracle import GrammarChoice          # noqa: F401  (re-exported: the constrained choice)


class PlainChoice:
    """The reference's greedy choice: argmax of the log-probabilities (lowest index on ties), no state."""

    def init(self, rows):
        return torch.zeros(rows, dtype=torch.long)

    def pick(self, logp, state):
        return torch.argmax(logp, dim=-1), state, None


def summarise(weights, ran):
    """weights (..., T) float32, ran (...) bool -> dict of float64 / int64 summaries with the fills where `ran` is false."""
    w = weights.to(torch.float64)
    T = w.shape[-1]
    peak = torch.argmax(w, dim=-1)                           # (the first maximal value: the lowest index)
    weight = w.gather(-1, peak.unsqueeze(-1)).squeeze(-1)
    centroid = (w * torch.arange(T, dtype=torch.float64)).sum(-1)
    return dict(peak=torch.where(ran, peak, torch.full_like(peak, -1)), weight=torch.where(ran, weight, torch.zeros_like(weight)),
                centroid=torch.where(ran, centroid, torch.full_like(centroid, -1.0)), weights=weights, ran=ran)


def decode_notes(enc, hidden, P, prefix, max_steps, choice, gt):
    """model_ref.decode_notes in evaluation mode (no dropout): greedy with the choice delegated (gt None), or every step fed from gt.
    -> log-probs (B, max_steps, V), lengths (B,), emitted / consumed ids (B, max_steps; <pad> where no step ran), weights (B, max_steps, T), steps run."""
    Bn, T = enc.shape[0], enc.shape[1]
    emb_w = P[prefix + ".embedding.weight"]
    token = F.embedding(torch.full((Bn, 1), SOS, dtype=torch.long), emb_w)
    probs = [None] * max_steps
    eos_seen = torch.zeros(Bn)
    lengths = torch.full((Bn,), max_steps, dtype=torch.long)
    ids = torch.full((Bn, max_steps), PAD, dtype=torch.long)
    weights = torch.zeros(Bn, max_steps, T)
    state = choice.init(Bn) if gt is None else None
    steps = 0
    for t in range(max_steps):
        if eos_seen.sum() == Bn:
            break
        steps = t + 1
        a = model_ref.attention(hidden, enc, P, prefix + ".attn").unsqueeze(1)
        weights[:, t] = a[:, 0]
        context = torch.bmm(a, enc)
        x = torch.cat([token, context], dim=2)
        h = model_ref.gru_cell(x[:, 0], hidden[0], P[prefix + ".gru.weight_ih_l0"], P[prefix + ".gru.weight_hh_l0"],
                               P[prefix + ".gru.bias_ih_l0"], P[prefix + ".gru.bias_hh_l0"])
        hidden = h.unsqueeze(0)
        out = torch.cat([h.unsqueeze(1), context], dim=-1)
        logits = out @ P[prefix + ".out.weight"].t() + P[prefix + ".out.bias"]
        prob = F.log_softmax(logits, dim=-1)
        probs[t] = prob.squeeze(1)
        if gt is not None:
            fed = gt[:, t]
        else:
            fed, state, _ = choice.pick(prob[:, 0], state)
        ids[:, t] = fed
        token = F.embedding(fed.unsqueeze(1), emb_w)
        for b in range(Bn):
            if int(fed[b]) == EOS:
                eos_seen[b] = 1
                lengths[b] = t + 1
    zero = enc.new_zeros(Bn, VOCAB_SIZE)
    score = torch.stack([p if p is not None else zero for p in probs], dim=1)
    return score, lengths, ids, weights, steps


def forward(P, B, cfg, spectrogram, choice=None, ground_truth=None):
    """model_ref.forward in evaluation mode with the attention rows recorded.  ground_truth None: inference with `choice` (default PlainChoice);
    otherwise the six ground-truth tensors, consumed at every note step and every bar (teacher_forcing_ratio = 1).
    -> (ts, key, up, lo) log-probs, decoded = {"up": (ids (B, bars, U), lengths (B, bars)), "lo": ...}, align = {"bar" | "up" | "lo": summarise(...)}."""
    choice = PlainChoice() if choice is None else choice
    with torch.no_grad():
        conv = model_ref.convstack_forward(spectrogram, P, B, False, True)
        enc, hidden = model_ref.encoder_forward(conv, P)
        Bn = enc.shape[0]
        if ground_truth is not None:
            ts_gt, key_gt, up_gt, up_len_gt, lo_gt, lo_len_gt = ground_truth
        sos_eos = torch.tensor([[SOS, EOS]], dtype=torch.long).repeat(Bn, 1)
        staff0 = model_ref._staff_token(sos_eos, torch.full((Bn,), 2), P)
        ts_tok = F.embedding(torch.full((Bn, 1), cfg["num_time_sig"], dtype=torch.long), P["decoder.time_sig_emb.weight"])
        key_tok = F.embedding(torch.full((Bn, 1), cfg["num_keys"], dtype=torch.long), P["decoder.key_emb.weight"])
        token = torch.cat([staff0, staff0, ts_tok, key_tok], dim=-1)

        def head(x, name):
            for i in (0, 2, 4):
                x = x @ P[f"decoder.{name}.{i}.weight"].t() + P[f"decoder.{name}.{i}.bias"]
                if i != 4:
                    x = torch.relu(x)
            return F.log_softmax(x, dim=-1)

        outs = {k: [] for k in ("ts", "key", "up", "lo", "up_ids", "lo_ids", "up_len", "lo_len", "up_w", "lo_w", "up_ran", "lo_ran", "bar_w")}
        U, L = cfg["max_length"]
        for bar in range(cfg["max_bars"]):
            a = model_ref.attention(hidden, enc, P, "decoder.attn").unsqueeze(1)
            context = torch.bmm(a, enc)
            x = torch.cat([token, context], dim=2)
            h = model_ref.gru_cell(x[:, 0], hidden[0], P["decoder.gru.weight_ih_l0"], P["decoder.gru.weight_hh_l0"],
                                   P["decoder.gru.bias_ih_l0"], P["decoder.gru.bias_hh_l0"])
            hidden = h.unsqueeze(0)
            bar_summary = h.unsqueeze(1)
            gt_u = up_gt[:, bar, :] if ground_truth is not None else None
            gt_l = lo_gt[:, bar, :] if ground_truth is not None else None
            up_probs, up_len, up_ids, up_w, up_n = decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.upper_decoder", U, choice, gt_u)
            lo_probs, lo_len, lo_ids, lo_w, lo_n = decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.lower_decoder", L, choice, gt_l)
            head_in = torch.cat([bar_summary.squeeze(1), context.squeeze(1)], dim=1)
            ts_lp = head(head_in, "time_sig_out")
            key_lp = head(head_in, "key_out")
            for k, v in (("ts", ts_lp), ("key", key_lp), ("up", up_probs), ("lo", lo_probs), ("up_ids", up_ids), ("lo_ids", lo_ids),
                         ("up_len", up_len), ("lo_len", lo_len), ("up_w", up_w), ("lo_w", lo_w), ("bar_w", a[:, 0]),
                         ("up_ran", (torch.arange(U) < up_n).expand(Bn, U)), ("lo_ran", (torch.arange(L) < lo_n).expand(Bn, L))):
                outs[k].append(v)
            if ground_truth is not None:
                up_tok = model_ref._staff_token(up_gt[:, bar, :], up_len_gt[:, bar], P)
                lo_tok = model_ref._staff_token(lo_gt[:, bar, :], lo_len_gt[:, bar], P)
                ts_tok = F.embedding(ts_gt[:, bar], P["decoder.time_sig_emb.weight"]).unsqueeze(1)
                key_tok = F.embedding(key_gt[:, bar], P["decoder.key_emb.weight"]).unsqueeze(1)
            else:
                up_tok = model_ref._staff_token(up_ids, up_len, P)
                lo_tok = model_ref._staff_token(lo_ids, lo_len, P)
                ts_tok = F.embedding(torch.argmax(ts_lp, dim=-1), P["decoder.time_sig_emb.weight"]).unsqueeze(1)
                key_tok = F.embedding(torch.argmax(key_lp, dim=-1), P["decoder.key_emb.weight"]).unsqueeze(1)
            token = torch.cat([up_tok, lo_tok, ts_tok, key_tok], dim=-1)
        st = {k: torch.stack(v, dim=1) for k, v in outs.items()}
    decoded = {"up": (st["up_ids"], st["up_len"]), "lo": (st["lo_ids"], st["lo_len"])}
    align = {"bar": summarise(st["bar_w"], torch.ones(st["bar_w"].shape[:2], dtype=torch.bool)),
             "up": summarise(st["up_w"], st["up_ran"]), "lo": summarise(st["lo_w"], st["lo_ran"])}
    return (st["ts"], st["key"], st["up"], st["lo"]), decoded, align
