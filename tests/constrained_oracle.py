"""TEST INFRASTRUCTURE: the CPU oracle's greedy decoder with the token choice as a parameter.

`oracle.model_ref.forward(..., inference=True)` chooses `argmax(log_softmax(logits))` inside its two decode loops.  This helper composes the
same parts of `oracle.model_ref` (convstack_forward, encoder_forward, attention, gru_cell, _staff_token) into the same two loops, operation
for operation, and hands the choice to a `GrammarChoice`: the legal token with the largest log-probability in the row's automaton state
(lowest index on ties), the state then moves along the table.  With `KernGrammar.permissive` that IS the reference's greedy decoder
(tests/test_kern_grammar_cpu.py asserts `torch.equal` on all four outputs); with the real grammar it is what the constrained HIP decoder
is compared against.  The returned log-probabilities are the model's unconstrained ones in either case."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import model_ref
from oracle.model_ref import EOS, PAD, SOS, VOCAB_SIZE


class GrammarChoice:
    """Masked argmax under a kern_grammar.KernGrammar (or its permissive stand-in) + the per-row automaton state."""

    def __init__(self, grammar):
        self.table = torch.from_numpy(np.asarray(grammar.table)).to(torch.long)      # (n_states, V)
        self.start = grammar.start

    def init(self, rows):
        return torch.full((rows,), self.start, dtype=torch.long)

    def pick(self, logp, state):
        """logp (rows, V), state (rows,) -> ids, new state, gap between the two best LEGAL candidates (inf where only one token is legal)."""
        nxt = self.table[state]                                                      # (rows, V)
        masked = logp.masked_fill(nxt < 0, float("-inf"))
        ids = torch.argmax(masked, dim=-1)
        if masked.shape[-1] > 1:
            top = torch.topk(masked, 2, dim=-1).values
            gap = top[:, 0] - top[:, 1]
        else:
            gap = torch.full((logp.shape[0],), float("inf"))
        return ids, nxt.gather(1, ids.unsqueeze(1)).squeeze(1), gap


def decode_notes(enc, hidden, P, prefix, max_steps, choice):
    """model_ref.decode_notes in inference mode (no dropout, no teacher forcing), token choice delegated.
    -> log-probs (B, max_steps, V), lengths (B,), emitted ids (B, max_steps; <pad> where no step ran), gaps (B, max_steps; inf where no step ran)."""
    Bn = enc.shape[0]
    emb_w = P[prefix + ".embedding.weight"]
    token = F.embedding(torch.full((Bn, 1), SOS, dtype=torch.long), emb_w)
    probs = [None] * max_steps
    eos_seen = torch.zeros(Bn)
    lengths = torch.full((Bn,), max_steps, dtype=torch.long)
    ids = torch.full((Bn, max_steps), PAD, dtype=torch.long)
    gaps = torch.full((Bn, max_steps), float("inf"))
    state = choice.init(Bn)
    for t in range(max_steps):
        if eos_seen.sum() == Bn:
            break
        a = model_ref.attention(hidden, enc, P, prefix + ".attn").unsqueeze(1)
        context = torch.bmm(a, enc)
        x = torch.cat([token, context], dim=2)
        h = model_ref.gru_cell(x[:, 0], hidden[0], P[prefix + ".gru.weight_ih_l0"], P[prefix + ".gru.weight_hh_l0"],
                               P[prefix + ".gru.bias_ih_l0"], P[prefix + ".gru.bias_hh_l0"])
        hidden = h.unsqueeze(0)
        out = torch.cat([h.unsqueeze(1), context], dim=-1)
        logits = out @ P[prefix + ".out.weight"].t() + P[prefix + ".out.bias"]
        prob = F.log_softmax(logits, dim=-1)
        probs[t] = prob.squeeze(1)
        am, state, gaps[:, t] = choice.pick(prob[:, 0], state)
        ids[:, t] = am
        token = F.embedding(am.unsqueeze(1), emb_w)
        for b in range(Bn):
            if int(am[b]) == EOS:
                eos_seen[b] = 1
                lengths[b] = t + 1
    zero = enc.new_zeros(Bn, VOCAB_SIZE)
    score = torch.stack([p if p is not None else zero for p in probs], dim=1)
    return score, lengths, ids, gaps


def forward(P, B, cfg, spectrogram, choice):
    """model_ref.forward(..., inference=True, training=False) with the token choice delegated.
    -> (ts, key, up, lo) log-probs, decoded = {"up": (ids (B, bars, U), lengths (B, bars)), "lo": ...}, gaps = {"up": (B, bars, U), "lo": ...}."""
    with torch.no_grad():
        conv = model_ref.convstack_forward(spectrogram, P, B, False, True)
        enc, hidden = model_ref.encoder_forward(conv, P)
        Bn = enc.shape[0]
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

        outs = {k: [] for k in ("ts", "key", "up", "lo", "up_ids", "lo_ids", "up_len", "lo_len", "up_gap", "lo_gap")}
        U, L = cfg["max_length"]
        for bar in range(cfg["max_bars"]):
            a = model_ref.attention(hidden, enc, P, "decoder.attn").unsqueeze(1)
            context = torch.bmm(a, enc)
            x = torch.cat([token, context], dim=2)
            h = model_ref.gru_cell(x[:, 0], hidden[0], P["decoder.gru.weight_ih_l0"], P["decoder.gru.weight_hh_l0"],
                                   P["decoder.gru.bias_ih_l0"], P["decoder.gru.bias_hh_l0"])
            hidden = h.unsqueeze(0)
            bar_summary = h.unsqueeze(1)
            up_probs, up_len, up_ids, up_gap = decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.upper_decoder", U, choice)
            lo_probs, lo_len, lo_ids, lo_gap = decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.lower_decoder", L, choice)
            head_in = torch.cat([bar_summary.squeeze(1), context.squeeze(1)], dim=1)
            ts_lp = head(head_in, "time_sig_out")
            key_lp = head(head_in, "key_out")
            for k, v in (("ts", ts_lp), ("key", key_lp), ("up", up_probs), ("lo", lo_probs), ("up_ids", up_ids), ("lo_ids", lo_ids),
                         ("up_len", up_len), ("lo_len", lo_len), ("up_gap", up_gap), ("lo_gap", lo_gap)):
                outs[k].append(v)
            up_tok = model_ref._staff_token(up_ids, up_len, P)
            lo_tok = model_ref._staff_token(lo_ids, lo_len, P)
            ts_tok = F.embedding(torch.argmax(ts_lp, dim=-1), P["decoder.time_sig_emb.weight"]).unsqueeze(1)
            key_tok = F.embedding(torch.argmax(key_lp, dim=-1), P["decoder.key_emb.weight"]).unsqueeze(1)
            token = torch.cat([up_tok, lo_tok, ts_tok, key_tok], dim=-1)
        st = {k: torch.stack(v, dim=1) for k, v in outs.items()}
    decoded = {"up": (st["up_ids"], st["up_len"]), "lo": (st["lo_ids"], st["lo_len"])}
    gaps = {"up": st["up_gap"], "lo": st["lo_gap"]}
    return (st["ts"], st["key"], st["up"], st["lo"]), decoded, gaps
