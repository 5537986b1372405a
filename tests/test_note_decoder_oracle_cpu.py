"""CPU side of tests/test_gpu_note_decoder_call.py: the float64 oracle of one note-decoder call (tests/note_decoder_oracle.py) tied to the project's
existing port of the reference (oracle/model_ref.decode_notes), and the PRECONDITIONS of every GPU case, checked where no GPU is needed: the argmax
margins of the inputs (a condition on the inputs, not a tolerance: the g2 fixture states the same as `min_margin`) and the properties of the row plans."""
import pytest
import torch

from oracle import model_ref
from tests import note_decoder_oracle as oracle
from tests import test_gpu_note_decoder_call as gpu

PLANNED = [c for c in gpu.CASES if c.planned is True]


class _Coins:
    """rng stub of model_ref.decode_notes: random() returns the listed values, one per executed step."""
    def __init__(self, values):
        self.values = list(values)

    def random(self):
        return self.values.pop(0)


def _small(rows=5, T=13, seed=3):
    g = torch.Generator().manual_seed(seed)
    W = gpu._weights()
    U = gpu.cfg()["max_length"][0]
    enc = torch.tanh(torch.randn(rows, T, 2 * gpu.H, generator=g))
    h0 = torch.tanh(torch.randn(rows, 2 * gpu.H, generator=g))
    gt = torch.randint(0, 145, (rows, U), generator=g)
    gt[0, 3] = gt[0, 9] = gt[2, 5] = model_ref.EOS           # (two rows show <eos>, one of them twice; the others never: the loop runs all U steps)
    return W, enc, h0, gt, U


def _P64(W):
    return {gpu.PREFIX + k: v.double() for k, v in W.items()}


@pytest.mark.parametrize("coins", ["alternating", "all forced", "none forced"])
def test_oracle_equals_the_port_of_the_reference(coins):
    """Flags all-ones or all-zeros per step, one bar, no `until`: probabilities and lengths of model_ref.decode_notes in float64, to 1e-12."""
    W, enc, h0, gt, U = _small()
    forced = {"alternating": [t % 3 != 1 for t in range(U)], "all forced": [True] * U, "none forced": [False] * U}[coins]
    ref_p, ref_len = model_ref.decode_notes(enc.double(), h0.double().unsqueeze(0), _P64(W), gpu.PREFIX, U, False, gt, 0.5, False,
                                            _Coins([0.0 if f else 1.0 for f in forced]), False)
    f = oracle.decode_call(W, enc, h0, gt, [int(f) for f in forced], 1, enc.shape[0], U, U)
    assert f["steps"] == U
    assert float((f["probs"] - ref_p).abs().max()) <= 1e-12
    assert torch.equal(f["lengths"], ref_len)
    assert torch.equal(f["ids"], ref_p.argmax(-1))


def test_greedy_oracle_equals_the_port_of_the_reference():
    g = gpu.GREEDY[0]
    i = gpu.greedy_inputs(g.rows, g.T, g.seed)
    U = i["U"]
    ref_p, ref_len = model_ref.decode_notes(i["enc"].double(), i["h0"].double().unsqueeze(0), _P64(i["W"]), gpu.PREFIX, U, True, None, 0, False, _Coins([1.0] * U), False)
    f = oracle.decode_call(i["W"], i["enc"], i["h0"], None, None, 1, g.rows, U, U)
    n = f["steps"]
    assert n < U, "the case should end before the cap: every row emits <eos>"
    assert float((f["probs"] - ref_p[:, :n]).abs().max()) <= 1e-12 and float(ref_p[:, n:].abs().max()) == 0.0
    assert torch.equal(f["lengths"], ref_len)


def test_saved_tensors_rebuild_the_state():
    """The per-step tensors in the layouts the library saves are consistent with each other: gates = [r | z | n | gh_n], x = [token | ctx] and
    o = [h' | ctx] rebuild h by the GRU formula (torch.nn.GRU), q is the query Linear of the state, attw sums to one."""
    W, enc, h0, gt, U = _small()
    n, H2, E = 6, 2 * gpu.H, gpu.E
    f = oracle.decode_call(W, enc, h0, gt, [1, 0, 1, 1, 0, 0], 1, enc.shape[0], n, U)
    Wd = {k: v.double() for k, v in W.items()}
    for t in range(n):
        r, z, ng, ghn = f["gates"][t].split(H2, dim=1)
        x, h, hn = f["x"][t], f["h"][t], f["h"][t + 1]
        gi_n = x @ Wd[".gru.weight_ih_l0"][2 * H2:].t() + Wd[".gru.bias_ih_l0"][2 * H2:]
        assert float((torch.tanh(gi_n + r * ghn) - ng).abs().max()) <= 1e-12
        assert float(((1 - z) * ng + z * h - hn).abs().max()) <= 1e-12
        assert float((ghn - (h @ Wd[".gru.weight_hh_l0"][2 * H2:].t() + Wd[".gru.bias_hh_l0"][2 * H2:])).abs().max()) <= 1e-12
        assert torch.equal(f["o"][t][:, :H2], hn) and torch.equal(f["o"][t][:, H2:], x[:, E:])
        assert float((f["q"][t] - (h @ Wd[".attn.attn.weight"][:, :H2].t() + Wd[".attn.attn.bias"])).abs().max()) <= 1e-12
        assert float((f["attw"][t].sum(1) - 1).abs().max()) <= 1e-12
        tok = torch.full((x.shape[0],), model_ref.SOS) if t == 0 else f["fed"][:, t - 1]
        assert torch.equal(x[:, :E], Wd[".embedding.weight"][tok])
    assert torch.equal(f["x"][n][:, :E], Wd[".embedding.weight"][f["fed"][:, n - 1]])
    assert torch.equal(f["fed"][:, 0], gt[:, 0]) and torch.equal(f["fed"][:, 1], f["ids"][:, 1])


def test_key_projection_is_a_leaf():
    """dK and dEnc as the call returns them: the chain rule through K = enc W_e^T (what Backward.finish adds: dW_e += dK^T enc, dEnc += dK W_e) turns
    them into the gradients of the graph in which enc feeds the keys too; the call's own attn.attn.weight gradient is zero in its key half."""
    W, enc, h0, gt, U = _small(rows=3, T=7)
    n, H2 = 4, 2 * gpu.H
    g = torch.Generator().manual_seed(1)
    dprobs = torch.randn(3, n, gpu.V, generator=g, dtype=torch.float64)
    f = oracle.decode_call(W, enc, h0, gt, [1, 0, 0, 1], 1, 3, n, U, grad=True)
    got = oracle.call_backward(f, dprobs)
    assert float(got["params"][".attn.attn.weight"][:, H2:].abs().max()) == 0.0 and float(got["dK"].abs().max()) > 0
    # the same call through model_ref.decode_notes, enc a leaf that feeds keys and contexts alike
    P = {k: v.clone().requires_grad_(True) for k, v in _P64(W).items()}
    e = enc.double().clone().requires_grad_(True)
    ref_p, _ = model_ref.decode_notes(e, h0.double().unsqueeze(0), P, gpu.PREFIX, n, False, gt, 0.5, False, _Coins([0.0, 1.0, 1.0, 0.0]), False)
    torch.autograd.backward(ref_p, dprobs)
    We = W[".attn.attn.weight"].double()[:, H2:]
    full_enc = got["dEnc"] + got["dK"] @ We
    full_w = got["params"][".attn.attn.weight"].clone()
    full_w[:, H2:] += torch.einsum("bth,btk->hk", got["dK"], enc.double())
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    assert rel(full_enc, e.grad) <= 1e-11 and rel(full_w, P[gpu.PREFIX + ".attn.attn.weight"].grad) <= 1e-11


def test_finished_rows_contribute_nothing():
    """Rows are independent: with dprobs zero behind `until`, what a finished row goes on to consume and compute changes no gradient."""
    c = PLANNED[0]
    i = gpu.case_inputs(c)
    dead = ~oracle.live_pairs(i["until"], i["R"], i["U"])
    other = torch.where(dead, torch.randint(0, 145, i["gt"].shape, generator=torch.Generator().manual_seed(2)), i["gt"])
    assert not torch.equal(other, i["gt"])
    res = []
    for gt in (i["gt"], other):
        f = oracle.decode_call(i["W"], i["enc"], i["h0"], gt, i["flags"], c.bars, c.clips, c.n, i["U"], grad=True)
        res.append(oracle.call_backward(f, i["dprobs"], i["until"]))
    for name, x, y in oracle.grad_views(*res):
        assert float((x - y).abs().max()) <= 1e-14 * float(x.abs().max()), name


# ------------------------------------------------------------------------------------------- preconditions of the GPU cases
@pytest.mark.parametrize("c", gpu.CASES, ids=[c.name for c in gpu.CASES])
def test_argmax_margin_of_every_training_case(c):
    """Every decision the float64 run takes at a live (row, step) pair -- the fed-back ones, which steer the rest of the row, and the merely reported
    ones, which the GPU test compares exactly as well -- has a top-2 log-probability gap of at least 1e-3."""
    i = gpu.case_inputs(c)
    with torch.no_grad():
        f = oracle.decode_call(i["W"], i["enc"], i["h0"], i["gt"], i["flags"], c.bars, c.clips, c.n, i["U"])
    live = oracle.live_pairs(i["until"], i["R"], c.n)
    consumed = torch.cat([live[:, 1:], torch.zeros(i["R"], 1, dtype=torch.bool)], dim=1)        # a decision is consumed by the row's next live step
    fed_back = f["fed_back"] & consumed
    assert int(fed_back.sum()) > 0, "no decision is fed back"
    m_fb, m_all = float(f["margin"][fed_back].min()), float(f["margin"][live].min())
    print(f"{c.name}: {int(fed_back.sum())} fed-back decisions, min margin {m_fb:.2e}; {int(live.sum())} live decisions, min margin {m_all:.2e}")
    assert m_fb >= gpu.MIN_MARGIN and m_all >= gpu.MIN_MARGIN
    # teacher forcing: one step forces every bar, one none; bars > 1: some step mixes
    full = (1 << c.bars) - 1
    assert full in i["flags"][:-1] and 0 in i["flags"][:-1]
    assert c.bars == 1 or any(0 < fl < full for fl in i["flags"])


@pytest.mark.parametrize("g", gpu.GREEDY, ids=[g.name for g in gpu.GREEDY])
def test_argmax_margin_of_every_greedy_case(g):
    i = gpu.greedy_inputs(g.rows, g.T, g.seed)
    with torch.no_grad():
        f = oracle.decode_call(i["W"], i["enc"], i["h0"], None, None, 1, g.rows, i["U"], i["U"])
    m = float(f["margin"].min())
    print(f"{g.name}: {f['steps']} steps, lengths {f['lengths'].tolist()}, min margin {m:.2e}")
    assert m >= gpu.MIN_MARGIN
    assert 1 < f["steps"] < i["U"], "the loop should end early, on the last row's <eos>"


@pytest.mark.parametrize("c", PLANNED, ids=[c.name for c in PLANNED])
def test_row_plans_are_the_engines(c):
    """The plan of a GPU case is what Engine.forward builds from the targets (decode_plan.row_limits -> staff_rows) and exercises what the plan exists
    for: rows that end after one step and rows that run to the end, clips that drop out, the prefix products, the tile sizes on both sides."""
    from piano_a2s_amd import decode_plan
    from piano_a2s_amd.spec import PAD
    i = gpu.case_inputs(c)
    n, R = c.n, i["R"]
    until = i["until"].view(c.bars, c.clips)
    gt = i["gt"].view(c.bars, c.clips, -1)
    assert torch.equal(decode_plan.row_limits(gt).to(torch.int32), until), "until = the index of each row's last non-<pad> target + 1"
    assert bool((gt[..., n:] == PAD).all())
    p = decode_plan.staff_rows(until, n)
    flat = p["until"]
    assert int((flat == 1).sum()) >= 1 and int((flat == n).sum()) >= 1
    assert p["n_active"][0] == c.clips and any(a > b for a, b in zip(p["n_active"][:-1], p["n_active"][1:])), p["n_active"]
    assert any(0 < 2 * m <= c.clips for m in p["m_active"]), p["m_active"]              # a2s_prefix_rows_ok
    rows = p["n_rows_active"]
    assert rows[0] == R and rows == [int((flat > t).sum()) for t in range(n)]
    for tile in (16, 64):
        if R > tile:            # (a call of fewer rows cannot stand on both sides)
            assert any(r > tile for r in rows) and any(0 < r < tile for r in rows), (tile, rows)
    if R > 160:                 # (above 160 rows the few-row path hands a launch to the mid-size kernels: one such launch must run through a `rowmap`)
        assert any(160 < r < R for r in rows), rows
    assert torch.equal(oracle.live_pairs(i["until"], R, n).reshape(-1).nonzero().squeeze(1).sort()[0],
                       (p["live_idx"].long() % R * n + p["live_idx"].long() // R).sort()[0])         # live_idx is step-major, live_pairs row-major
