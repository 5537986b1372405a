"""TEST INFRASTRUCTURE: the CPU oracle's note decoder under beam search, optionally under the kern grammar.

Composed from the parts of `oracle.model_ref` the way tests/constrained_oracle.py is; the K beam slots of a clip are extra batch rows
(row = slot * B + clip).  One `decode_notes` call is one bar and one staff; beams are local to it; at its end each clip keeps its best
hypothesis and the bar level goes on from that as in the greedy decoders.

Semantics (the specification the HIP kernels follow too):
  * slot 0 starts at score 0, the others at -inf: dead, which counts as finished;
  * a live, unfinished slot k offers every token v at score_k + log_softmax(logits_k)[v] (ONE fp32 add), -inf where the grammar forbids v in
    the slot's state; a finished slot offers exactly (k, <pad>) at its own score;
  * the new beam: the K candidates with the largest scores, ties to the lowest flat index k * V + v, best first;
  * a new slot inherits its parent's finished flag, or is finished by <eos>, or is dead at -inf; its automaton state moves along the table
    unless the parent was finished (or the token is illegal: dead anyway);
  * the loop ends before the step at which every slot of every clip is finished, or at max_steps;
  * pick: largest score / len^alpha (alpha = 0: the raw score), len = index of <eos> + 1 or the steps executed; ties to the lowest slot;
  * probs[t] = the UNCONSTRAINED log_softmax computed at step t in the slot the winner's lineage occupied then.
Two margins come back with every call: the smallest gap between the K-th kept and the best dropped candidate over all steps and clips, and
the smallest gap between a clip's best and second-best final hypothesis."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import model_ref
from oracle.model_ref import EOS, PAD, SOS, VOCAB_SIZE

NEG = float("-inf")


def select(scores, finished, states, lp, table, K, pad=PAD, eos=EOS):
    """One clip, one step.  scores (K,) float32, finished (K,) bool, states (K,) int, lp (K, V) float32 numpy; table (n_states, V) or None.
    -> token, parent, score, state, finished (length-K lists, best first) and the gap between the K-th kept and the best dropped candidate."""
    V = lp.shape[1]
    cands = []
    for k in range(K):
        if finished[k]:
            cands.append((np.float32(scores[k]), k * V + pad))
            continue
        for v in range(V):
            legal = table is None or table[states[k]][v] >= 0
            cands.append((np.float32(scores[k]) + np.float32(lp[k, v]) if legal else np.float32(NEG), k * V + v))
    cands.sort(key=lambda c: (-float(c[0]), c[1]))
    kept, dropped = cands[:K], cands[K:]
    gap = float("inf")
    if dropped and float(kept[-1][0]) > NEG and float(dropped[0][0]) > NEG:
        gap = float(kept[-1][0]) - float(dropped[0][0])
    out = ([], [], [], [], [])
    for sc, flat in kept:
        par, tok = divmod(flat, V)
        st = states[par]
        if table is not None and not finished[par] and table[st][tok] >= 0:
            st = int(table[st][tok])
        fin = bool(finished[par]) or tok == eos or not float(sc) > NEG
        for lst, val in zip(out, (tok, par, np.float32(sc), st, fin)):
            lst.append(val)
    return out + (gap,)


def pick(scores, lens, alpha):
    """-> winning slot (largest score / len^alpha, ties to the lowest slot) and the gap to the runner-up (inf where there is none alive)."""
    norm = [float(s) if alpha == 0 or l <= 0 else float(np.float32(s) / np.float32(np.power(np.float32(l), np.float32(alpha)))) for s, l in zip(scores, lens)]
    order = sorted(range(len(norm)), key=lambda k: (-norm[k], k))
    gap = float("inf")
    if len(order) > 1 and norm[order[1]] > NEG:
        gap = norm[order[0]] - norm[order[1]]
    return order[0], gap


def backtrack(tokens, parents, slot, T, eos=EOS):
    """Walk slot `slot` back over T steps -> its tokens (T,), the slot its lineage occupied DURING each step (T,), index of its <eos> or -1."""
    ids, rows, e = [0] * T, [0] * T, -1
    cur = slot
    for t in range(T - 1, -1, -1):
        ids[t] = int(tokens[t][cur])
        if ids[t] == eos:
            e = t
        cur = int(parents[t][cur])
        rows[t] = cur
    return ids, rows, e


def decode_notes(enc, hidden, P, prefix, max_steps, K, grammar=None, alpha=0.0):
    """Beam search over one (bar, staff).  -> log-probs (B, max_steps, V), lengths (B,), ids (B, max_steps), scores (B,) float32,
    (step margin, final gap)."""
    Bn = enc.shape[0]
    R = K * Bn
    table = None if grammar is None else np.asarray(grammar.table)
    emb_w = P[prefix + ".embedding.weight"]
    enc_r = enc.repeat(K, 1, 1)
    hidden = hidden.repeat(1, K, 1)
    token = F.embedding(torch.full((R, 1), SOS, dtype=torch.long), emb_w)
    scores = np.full((K, Bn), NEG, dtype=np.float32)
    scores[0] = 0
    finished = np.ones((K, Bn), dtype=bool)
    finished[0] = False
    states = np.full((K, Bn), 0 if grammar is None else grammar.start, dtype=np.int64)
    scratch, tokens, parents = [], [], []
    step_margin = float("inf")
    for t in range(max_steps):
        if finished.all():
            break
        a = model_ref.attention(hidden, enc_r, P, prefix + ".attn").unsqueeze(1)
        context = torch.bmm(a, enc_r)
        x = torch.cat([token, context], dim=2)
        h = model_ref.gru_cell(x[:, 0], hidden[0], P[prefix + ".gru.weight_ih_l0"], P[prefix + ".gru.weight_hh_l0"],
                               P[prefix + ".gru.bias_ih_l0"], P[prefix + ".gru.bias_hh_l0"])
        out = torch.cat([h.unsqueeze(1), context], dim=-1)
        logits = out @ P[prefix + ".out.weight"].t() + P[prefix + ".out.bias"]
        lp = F.log_softmax(logits, dim=-1)[:, 0]                                       # (R, V)
        scratch.append(lp)
        lp_n = lp.numpy().reshape(K, Bn, -1)
        tok_t, par_t = np.zeros((K, Bn), dtype=np.int64), np.zeros((K, Bn), dtype=np.int64)
        new = (scores.copy(), states.copy(), finished.copy())
        for b in range(Bn):
            tok, par, sc, st, fin, gap = select(scores[:, b], finished[:, b], states[:, b], lp_n[:, b], table, K)
            step_margin = min(step_margin, gap)
            tok_t[:, b], par_t[:, b], new[0][:, b], new[1][:, b], new[2][:, b] = tok, par, sc, st, fin
        scores, states, finished = new
        tokens.append(tok_t)
        parents.append(par_t)
        src = torch.from_numpy(par_t.reshape(-1) * Bn + np.tile(np.arange(Bn), K))         # new row j * B + b <- row parent * B + b
        hidden = h[src].unsqueeze(0)
        token = F.embedding(torch.from_numpy(tok_t.reshape(-1, 1)), emb_w)
    T = len(tokens)
    probs = enc.new_zeros(Bn, max_steps, VOCAB_SIZE)
    ids = torch.full((Bn, max_steps), PAD, dtype=torch.long)
    lengths = torch.full((Bn,), max_steps, dtype=torch.long)
    best = torch.zeros(Bn)
    final_gap = float("inf")
    for b in range(Bn):
        walks = [backtrack([tk[:, b] for tk in tokens], [pr[:, b] for pr in parents], k, T) for k in range(K)]
        slot, gap = pick(scores[:, b], [w[2] + 1 if w[2] >= 0 else T for w in walks], alpha)
        final_gap = min(final_gap, gap)
        w_ids, w_rows, e = walks[slot]
        for t in range(T):
            ids[b, t] = w_ids[t]
            probs[b, t] = scratch[t][w_rows[t] * Bn + b]
        if e >= 0:
            lengths[b] = e + 1
        best[b] = float(scores[slot, b])
    return probs, lengths, ids, best, (step_margin, final_gap)


def forward(P, B, cfg, spectrogram, K, grammar=None, alpha=0.0):
    """model_ref.forward(..., inference=True, training=False) with both note decoders under beam search.
    -> (ts, key, up, lo) log-probs, decoded = {"up": (ids (B, bars, U), lengths (B, bars)), "lo": ...}, scores = {"up": (B, bars), "lo": ...},
    margins = (smallest step margin, smallest final gap) over every call."""
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

        outs = {k: [] for k in ("ts", "key", "up", "lo", "up_ids", "lo_ids", "up_len", "lo_len", "up_sc", "lo_sc")}
        margins = [float("inf"), float("inf")]
        U, L = cfg["max_length"]
        for bar in range(cfg["max_bars"]):
            a = model_ref.attention(hidden, enc, P, "decoder.attn").unsqueeze(1)
            context = torch.bmm(a, enc)
            x = torch.cat([token, context], dim=2)
            h = model_ref.gru_cell(x[:, 0], hidden[0], P["decoder.gru.weight_ih_l0"], P["decoder.gru.weight_hh_l0"],
                                   P["decoder.gru.bias_ih_l0"], P["decoder.gru.bias_hh_l0"])
            hidden = h.unsqueeze(0)
            bar_summary = h.unsqueeze(1)
            up_probs, up_len, up_ids, up_sc, up_m = decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.upper_decoder", U, K, grammar, alpha)
            lo_probs, lo_len, lo_ids, lo_sc, lo_m = decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.lower_decoder", L, K, grammar, alpha)
            margins = [min(margins[i], up_m[i], lo_m[i]) for i in (0, 1)]
            head_in = torch.cat([bar_summary.squeeze(1), context.squeeze(1)], dim=1)
            ts_lp = head(head_in, "time_sig_out")
            key_lp = head(head_in, "key_out")
            for k, v in (("ts", ts_lp), ("key", key_lp), ("up", up_probs), ("lo", lo_probs), ("up_ids", up_ids), ("lo_ids", lo_ids),
                         ("up_len", up_len), ("lo_len", lo_len), ("up_sc", up_sc), ("lo_sc", lo_sc)):
                outs[k].append(v)
            up_tok = model_ref._staff_token(up_ids, up_len, P)
            lo_tok = model_ref._staff_token(lo_ids, lo_len, P)
            ts_tok = F.embedding(torch.argmax(ts_lp, dim=-1), P["decoder.time_sig_emb.weight"]).unsqueeze(1)
            key_tok = F.embedding(torch.argmax(key_lp, dim=-1), P["decoder.key_emb.weight"]).unsqueeze(1)
            token = torch.cat([up_tok, lo_tok, ts_tok, key_tok], dim=-1)
        st = {k: torch.stack(v, dim=1) for k, v in outs.items()}
    decoded = {"up": (st["up_ids"], st["up_len"]), "lo": (st["lo_ids"], st["lo_len"])}
    return (st["ts"], st["key"], st["up"], st["lo"]), decoded, {"up": st["up_sc"], "lo": st["lo_sc"]}, tuple(margins)
