"""The host plan of the note decoders' backward pass, pure (host data in, host data out: no torch, no ctypes, no liba2s_hip.so): after the reverse loop
of one decode call (a2s_note_decoder_bwd), which of the products that nobody in the recurrence waits for run where, over which rows, with which operand
ranges, and which tensors they read; and how the two staves of a segment are issued.  engine_bwd._note_decoder_bwd allocates, launches and walks the
plan; Backward.decoder_group asks plan_staff_issue once per segment; neither decides anything itself.

A call has steps x rows (step, row) pairs.  Rows whose targets had run out were skipped by the forward pass and carry EXACT zero gradients from then
on; the pairs that ran are the call's live index (decode_plan.staff_rows: live_idx).  Three sides follow the reverse loop:
  "weights" -- the four weight-gradient products of PRODUCTS with their bias sums, over Rw rows: everything only the optimizer waits for;
  "keys"    -- the key / encoder-output gradients of the call's attention (engine_bwd._attn_deferred);
  "scatter" -- the embedding rows of the tokens each step consumed (a2s_embed_scatter_add), over the same Rw rows.
The kernels trust the operand ranges and the row count without checking, and the late closure reads tensors on another stream than the one that
allocated them: tests/test_dec_bwd_plan_cpu.py holds the planner to a literal restatement of the rules and the executor's wiring to this plan."""
from collections import namedtuple

GATHER_BELOW = 0.8          # the operands are gathered when fewer than this share of the call's (step, row) pairs ran (22 KB per pair, read once)


class Product(namedtuple("Product", "name x dy weight bias cols ld col0 x_bound dy_range")):
    """One weight-gradient product: G[prefix + weight][:, col0 : col0 + cols] += dy^T x over the call's Rw rows; G[prefix + bias] += colsum(dy).
    x, dy: operand names (see OPERANDS) of the layer's input and of the gradient of its output.  cols, ld: the input's width and the gradient matrix's
    leading dimension, as names dim() evaluates.  x_bound: the range handed to the two-term fp16 product for x -- "one" (a GRU state lies in (-1, 1)),
    "max(one, enc)" (o = [state | context], the context a convex combination of encoder rows), "max(emb, enc)" (x = [embedding row | context]).
    dy_range: "dlog_amax" -- max |dlog|, measured once before the reverse loop (the product that gates the recurrence takes it too) -- or "measure":
    a2s_absmax over the operand as the product reads it (gathered or not)."""


PRODUCTS = (
    Product("out", "o", "dlog", ".out.weight", ".out.bias", "4H", "4H", 0, "max(one, enc)", "dlog_amax"),
    Product("w_ih", "x", "dgi", ".gru.weight_ih_l0", ".gru.bias_ih_l0", "E+2H", "E+2H", 0, "max(emb, enc)", "measure"),
    Product("w_hh", "h", "dgh", ".gru.weight_hh_l0", ".gru.bias_hh_l0", "2H", "2H", 0, "one", "measure"),
    # the query half of the attention's (H, 4H) matrix: columns 0 .. 2H (the key half is Backward.finish's)
    Product("attn_q", "h", "dq", ".attn.attn.weight", ".attn.attn.bias", "2H", "4H", 0, "one", "measure"),
)
# every operand a product reads, (steps, rows, width) step-major, in the order the gather takes them: saved by the forward (o, x, h) or written before /
# by the reverse loop
OPERANDS = ("dlog", "o", "dgi", "dgh", "dq", "x", "h")
# what the scatter reads beside the live index: the token columns of dx; the tokens are rebuilt from ids, gt_bar and the teacher-forcing bits; the dropout mask
SCATTER_READS = ("dx", "ids", "gt_bar", "flags_dev", "drop")
# do_all is read by the reverse loop only; the late entry has always held it, so its block returns to the allocator when the closure has run, as before
HELD_BESIDE = ("do_all",)


def dim(name, H, E):
    """A width of PRODUCTS in floats."""
    return {"2H": 2 * H, "4H": 4 * H, "E+2H": E + 2 * H}[name]


def keep_alive(products=PRODUCTS):
    """The names of every tensor the "weights" and "scatter" sides read that the issuing stream allocated: with placement "late" they run on the
    weight-gradient stream, which must record each of them (a block handed back to the issuing stream early is a use-after-free that shows only under
    allocator pressure).  Derived from the product table and the scatter's operands; the parameters and the gradient buffers outlive the step."""
    names = []
    for p in products:
        names += [p.dy, p.x] + ([p.dy_range] if p.dy_range != "measure" else []) + (["enc_amax"] if "enc" in p.x_bound else [])
    names += list(SCATTER_READS) + ["live_idx"] + list(HELD_BESIDE)
    return tuple(dict.fromkeys(names))


KEEP_ALIVE = keep_alive()


class NoteDecBwdPlan(namedtuple("NoteDecBwdPlan", "gather rw empty placement on_stream in_closure products operands keep_alive")):
    """gather: the operands of "weights" and "scatter" are gathered at the call's live index first (dense operands of rw rows).
    rw: the rows every product contracts over and the scatter walks: the live pairs when gathered, else steps * rows.
    empty: a gathered call with rw == 0 -- nothing ran, every weight gradient of the call is zero: "weights" measures the embedding table's range (a
    launch the call has always made) and returns; see on_stream for what else is skipped.  (A call of zero steps is not gathered -- 0 < 0.8 * 0 is
    false -- and issues its products over zero rows, as it always has.)
    placement: "inline" -- all on the issuing stream; "late" -- "keys" on the issuing stream, then an event, then the rest as a closure Backward.finish
    runs on the weight-gradient stream beside the encoder's back-propagation.
    on_stream / in_closure: the sides in the order they are issued.  Inline, an empty call skips "keys" as well as "scatter" (the key side of a call
    in which nothing ran adds exact zeros); late, "keys" has been issued before the closure learns that the call is empty.
    products, operands: PRODUCTS, OPERANDS.  keep_alive: KEEP_ALIVE = keep_alive(), what a late entry holds and the weight-gradient stream records."""


def plan_note_decoder_bwd(steps, rows, live_steps, n_live, late):
    """steps, rows: the executed steps and the rows (groups * clips) of the call.  live_steps, n_live: the step count the live index was planned for and
    its length; n_live None: no live index (no row plan, or one planned without live rows).  late: the weight side goes to Backward.finish."""
    pairs = steps * rows          # (the product first: 0.8 * 3 * 5 is not 0.8 * 15 in floating point, and 12 live pairs of 15 sit on that edge)
    gather = n_live is not None and live_steps == steps and n_live < GATHER_BELOW * pairs
    rw = n_live if gather else pairs
    empty = gather and rw == 0
    if late:
        on_stream, in_closure = ("keys",), (("weights",) if empty else ("weights", "scatter"))
    else:
        on_stream, in_closure = (("weights",) if empty else ("weights", "keys", "scatter")), ()
    return NoteDecBwdPlan(gather, rw, empty, "late" if late else "inline", on_stream, in_closure, PRODUCTS, OPERANDS, KEEP_ALIVE)


def plan_staff_issue(concurrent, staves_concurrent, any_persist, has_pair, attn_pair_switch):
    """How a segment's two note decoders are issued.  concurrent: the forward ran the staves side by side; staves_concurrent: this clip group has two
    staff streams (engine.staves_concurrent); any_persist: a call of the group ran as a persistent launch (two of those must never be in flight together);
    has_pair: the forward planned the segment as a pair; attn_pair_switch: the library's attn_pair switch.
    "pair": one host loop for both staves, the attention sweep of a step as one launch (a2s_note_decoder_bwd_pair); "fork": one host thread and stream
    per staff; "serial": upper then lower on the current stream."""
    if not (concurrent and staves_concurrent and not any_persist):
        return "serial"
    return "pair" if has_pair and attn_pair_switch else "fork"
