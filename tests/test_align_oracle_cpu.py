"""The alignment CPU oracle (tests/align_oracle.py) and the host side of the alignment option, without a GPU:

the helper with the plain choice IS oracle.model_ref.forward(inference=True), with given ids it IS the oracle's teacher-forced forward (torch.equal
on all four outputs -- that validates the helper the GPU tests compare against); its recorded attention rows are what the issue says of the small
fixtures (not near-constants); the model's and the recipe's defaults; the C layout of a2s_align_args against its ctypes mirror."""
import ctypes as C
import json
import os
import subprocess
import types

import pytest
import torch

from oracle import model_ref
from piano_a2s_amd import spec, synthetic
from tests import align_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)


@pytest.fixture(scope="module")
def g1(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g1_small.json")))
    cfg = spec.default_cfg(**meta["cfg"])
    return meta, cfg, synthetic.make_batch(3, cfg, meta["batch_seed"], **SMALL_BATCH)


def _state(cfg, case):
    return spec.split_state(spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True))


@pytest.mark.parametrize("seed", [11, 18])
def test_plain_choice_is_the_reference_greedy_decoder(g1, seed):
    meta, cfg, batch = g1
    P, B = _state(cfg, meta["cases"][f"greedy_s{seed}"])
    ref = model_ref.forward(P, B, cfg, batch[0], inference=True)
    outs, decoded, align = align_oracle.forward(P, B, cfg, batch[0])
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), n
    frames = batch[0].shape[2]
    gaps = []
    for k, o in (("bar", None), ("up", outs[2]), ("lo", outs[3])):
        al = align[k]
        if o is not None:
            assert torch.equal(al["ran"], o.abs().sum(-1) > 0), "a step ran exactly where the reference wrote log-probabilities"
            assert torch.equal(decoded[k][0][al["ran"]], o.argmax(-1)[al["ran"]])
        ran = al["ran"]
        assert al["weights"].shape[-1] == frames and al["weights"].dtype == torch.float32
        assert torch.allclose(al["weights"][ran].sum(-1), torch.ones(int(ran.sum())), atol=1e-5), "softmax rows"
        assert (al["weights"][~ran] == 0).all() and (al["peak"][~ran] == -1).all() and (al["weight"][~ran] == 0).all() and (al["centroid"][~ran] == -1).all()
        c = al["centroid"][ran]
        assert float(c.min()) >= 0 and float(c.max()) <= frames - 1
        # the fixture exercises the alignment: the centroids move over the clip, the peaks take many frames
        span, peaks = float(c.max() - c.min()), len(set(al["peak"][ran].tolist()))
        top = torch.topk(al["weights"][ran].to(torch.float64), 2, dim=-1).values
        gaps.append(float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
        print(f"greedy_s{seed}.{k}: centroids {float(c.min()):.1f} .. {float(c.max()):.1f}, {peaks} distinct peaks, smallest relative top-2 gap {gaps[-1]:.3e}")
        assert span >= 5 and peaks >= 5
    assert min(gaps) > 2e-4, "fixture precondition of the GPU test: weights within 1e-4 cannot disagree on the peak"


def test_given_ids_is_the_reference_teacher_forced_forward(g1):
    meta, cfg, batch = g1
    P, B = _state(cfg, meta["cases"]["eval_tf1"])
    gt = list(batch[1:7])
    ref = model_ref.forward(P, B, cfg, batch[0], inference=False, ground_truth=gt, teacher_forcing_ratio=1.0, training=False)
    outs, decoded, align = align_oracle.forward(P, B, cfg, batch[0], ground_truth=gt)
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), n
    for k, g, o in (("up", gt[2], outs[2]), ("lo", gt[4], outs[3])):
        ran = align[k]["ran"]
        assert torch.equal(ran, o.abs().sum(-1) > 0)
        assert torch.equal(decoded[k][0][ran], g[ran]), "the consumed ids are the given ones"


def test_summaries_of_a_known_row():
    w = torch.zeros(2, 6)
    w[0, 1], w[0, 4] = 0.5, 0.5                         # a tie: the lowest index
    w[1, 5] = 1.0
    s = align_oracle.summarise(w, torch.tensor([True, True]))
    assert s["peak"].tolist() == [1, 5] and s["weight"].tolist() == [0.5, 1.0] and s["centroid"].tolist() == [2.5, 5.0]
    s = align_oracle.summarise(w, torch.tensor([False, True]))
    assert (s["peak"][0], s["weight"][0], s["centroid"][0]) == (-1, 0.0, -1.0)


def test_model_and_engine_defaults():
    import models
    from piano_a2s_amd import engine
    assert models.ScoreTranscription.alignment is False and models.ScoreTranscription.last_alignment is None
    eng = engine.Engine(spec.default_cfg())
    assert eng.alignment is False and eng.alignment_out is None


def test_recipe_refuses_the_option_for_a_module_without_it():
    """--alignment=true with a transcription module that has no `alignment` attribute: a clear ValueError; without the option nothing is touched."""
    from piano_a2s_amd import recipe

    def brain(module, **hp):
        b = object.__new__(recipe.ASR)
        b.hparams, b.modules = types.SimpleNamespace(**hp), types.SimpleNamespace(transcription=module)
        return b

    plain = torch.nn.Linear(2, 2)
    for on in (True, "true"):
        with pytest.raises(ValueError, match="alignment"):
            brain(plain, alignment=on)._set_constrained_decoding()
    for off in ({}, {"alignment": False}, {"alignment": "false"}):
        b = brain(plain, **off)
        b._set_constrained_decoding()
        assert not b._alignment() and not hasattr(plain, "alignment")
    capable = torch.nn.Linear(2, 2)
    capable.alignment = False
    brain(capable, alignment=True)._set_constrained_decoding()
    assert capable.alignment is True


def test_align_block_layout_matches_c(tmp_path):
    """sizeof / offsetof of a2s_align_args as the C compiler sees them == the ctypes mirror (the technique of tests/test_cabi.py)."""
    from piano_a2s_amd import hip
    cls = hip.AlignArgs
    fields = [f[0] for f in cls._fields_]
    src = tmp_path / "layout.c"
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(a2s_align_args, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "a2s.h"\nint main(){printf("sizeof %zu\\n", sizeof(a2s_align_args));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(cls)
    for f in fields:
        assert int(out[f]) == getattr(cls, f).offset, f
    header = open(os.path.join(ROOT, "include", "a2s.h")).read()
    block = header[header.index("typedef struct a2s_align_args"):header.index("} a2s_align_args;")]
    assert all(f in block for f in fields) and len(fields) == 8
