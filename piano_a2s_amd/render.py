"""Rendered synthetic corpus, device side: render programs -> 16 kHz waveforms (csrc/a2s_render.hip).

The host draws a score and its note events (piano_a2s_amd.scoregen) and packs them into a few kilobytes per clip; the waveform of every clip of the
batch is synthesised on the GPU in one launch and goes through the GPU VQT (piano_a2s_amd.vqt) into the model.  There is no CPU implementation in
the product (tests/render_oracle.py is the float64 definition the tests compare against)."""
import torch

from . import hip


def program_samples(programs):
    """n_samples of a batch of programs (word 0 of every header); the clips of a batch must agree.  On host programs this reads nothing from the
    device (the recipe asks before it uploads the batch); on device programs it is ONE small blocking read."""
    lo, hi = torch.stack(torch.aminmax(programs[:, 0, 0])).tolist()
    if lo != hi or lo < 1:
        raise hip.A2SError(f"render: the clips of a batch need one positive n_samples (got {lo} .. {hi})")
    return lo


def render(programs, n_samples=None):
    """programs: (B, 1 + E, 8) int32 on the device -> (B, n_samples) float32 waveforms.  n_samples None: read from the headers."""
    if not torch.is_tensor(programs) or not programs.is_cuda:
        raise hip.A2SError("render runs on the GPU only (no CPU implementation in the product)")
    programs = programs.contiguous()
    if programs.shape[0] == 0:
        n_samples = int(n_samples or 0)
    return hip.render_notes(programs, program_samples(programs) if n_samples is None else n_samples)
