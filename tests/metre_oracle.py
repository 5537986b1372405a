"""TEST INFRASTRUCTURE: the constrained CPU oracle (tests/constrained_oracle.py) under the metre of the bar.

`forward` is `constrained_oracle.forward` with two differences: the heads of a bar are evaluated BEFORE its note decoders (they depend only on the
bar summary and the context, so the four outputs cannot change), and the token choice of both note decoders is a `MetreChoice` bound to the bar's
time-signature arg-max.  `constrained_oracle.decode_notes` is reused as it is: its `state` is the syntax state, the metre states live in the choice
object, one `kern_grammar.MetreState` per row, and follow the host definition `KernMetre.step` token by token.  With `L = 0` for every row (the
`lengths` override) this is `constrained_oracle.forward` with `GrammarChoice` -- tests/test_kern_metre_cpu.py asserts `torch.equal`."""
import torch
import torch.nn.functional as F

from oracle import model_ref
from oracle.model_ref import EOS, SOS
from tests import constrained_oracle


class MetreChoice:
    """Masked argmax under a kern_grammar.KernMetre: the legal token with the largest log-probability (lowest index on ties)."""

    def __init__(self, metre, lengths=None):
        self.metre = metre
        self.lengths = lengths              # None: L from the bound time-signature ids; else a callable ts_id -> L (tests: lambda ts: 0)
        self.ts_ids = None
        self.rows = None

    def bind(self, ts_ids):
        self.ts_ids = [int(t) for t in ts_ids]
        return self

    def init(self, rows):
        assert self.ts_ids is not None and len(self.ts_ids) == rows
        self.rows = [self.metre.start(t) if self.lengths is None else self.metre.start(L=self.lengths(t)) for t in self.ts_ids]
        return torch.full((rows,), self.metre.grammar.start, dtype=torch.long)

    def pick(self, logp, state):
        """logp (rows, V), state (rows,) -> ids, new syntax state, gap between the two best LEGAL candidates (inf where only one token is legal)."""
        V = logp.shape[-1]
        mask = torch.zeros(logp.shape, dtype=torch.bool)
        for r, st in enumerate(self.rows):
            assert st.s == int(state[r])
            legal = self.metre.legal_tokens(st)
            assert legal, f"row {r}: no legal token in state {st.ints()} / {st.s}"
            mask[r, legal] = True
        masked = logp.masked_fill(~mask, float("-inf"))
        ids = torch.argmax(masked, dim=-1)
        top = torch.topk(masked, 2, dim=-1).values if V > 1 else None
        gap = top[:, 0] - top[:, 1] if top is not None else torch.full((logp.shape[0],), float("inf"))
        self.rows = [self.metre.step(st, int(v)) for st, v in zip(self.rows, ids)]
        return ids, torch.tensor([st.s for st in self.rows], dtype=torch.long), gap


def forward(P, B, cfg, spectrogram, choice):
    """-> (ts, key, up, lo) log-probs, decoded = {"up": (ids (B, bars, U), lengths (B, bars)), "lo": ...}, gaps = {"up", "lo", "ts": (B, bars) top-2 gap of
    the time-signature head}."""
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

        outs = {k: [] for k in ("ts", "key", "up", "lo", "up_ids", "lo_ids", "up_len", "lo_len", "up_gap", "lo_gap", "ts_gap")}
        U, L = cfg["max_length"]
        for bar in range(cfg["max_bars"]):
            a = model_ref.attention(hidden, enc, P, "decoder.attn").unsqueeze(1)
            context = torch.bmm(a, enc)
            x = torch.cat([token, context], dim=2)
            h = model_ref.gru_cell(x[:, 0], hidden[0], P["decoder.gru.weight_ih_l0"], P["decoder.gru.weight_hh_l0"],
                                   P["decoder.gru.bias_ih_l0"], P["decoder.gru.bias_hh_l0"])
            hidden = h.unsqueeze(0)
            bar_summary = h.unsqueeze(1)
            head_in = torch.cat([bar_summary.squeeze(1), context.squeeze(1)], dim=1)
            ts_lp = head(head_in, "time_sig_out")
            key_lp = head(head_in, "key_out")
            ts_top = torch.topk(ts_lp, 2, dim=-1).values
            choice.bind(torch.argmax(ts_lp, dim=-1).tolist())
            up_probs, up_len, up_ids, up_gap = constrained_oracle.decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.upper_decoder", U, choice)
            lo_probs, lo_len, lo_ids, lo_gap = constrained_oracle.decode_notes(enc, bar_summary.transpose(0, 1), P, "decoder.lower_decoder", L, choice)
            for k, v in (("ts", ts_lp), ("key", key_lp), ("up", up_probs), ("lo", lo_probs), ("up_ids", up_ids), ("lo_ids", lo_ids),
                         ("up_len", up_len), ("lo_len", lo_len), ("up_gap", up_gap), ("lo_gap", lo_gap), ("ts_gap", ts_top[:, 0] - ts_top[:, 1])):
                outs[k].append(v)
            up_tok = model_ref._staff_token(up_ids, up_len, P)
            lo_tok = model_ref._staff_token(lo_ids, lo_len, P)
            ts_tok = F.embedding(torch.argmax(ts_lp, dim=-1), P["decoder.time_sig_emb.weight"]).unsqueeze(1)
            key_tok = F.embedding(torch.argmax(key_lp, dim=-1), P["decoder.key_emb.weight"]).unsqueeze(1)
            token = torch.cat([up_tok, lo_tok, ts_tok, key_tok], dim=-1)
        st = {k: torch.stack(v, dim=1) for k, v in outs.items()}
    decoded = {"up": (st["up_ids"], st["up_len"]), "lo": (st["lo_ids"], st["lo_len"])}
    gaps = {"up": st["up_gap"], "lo": st["lo_gap"], "ts": st["ts_gap"]}
    return (st["ts"], st["key"], st["up"], st["lo"]), decoded, gaps
