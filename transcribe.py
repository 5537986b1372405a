#!/usr/bin/env python3
"""Transcribe recordings: ``python transcribe.py hparams/finetune.yaml --checkpoint PATH audio.wav [more.wav ...] [--downbeats FILE | --track_downbeats [--beats_per_bar {2,3,4}]] [--out DIR]
[--window_seconds S --hop_seconds S --batch_size N --constrained_decoding --metrical_decoding --beam_size K --beam_length_penalty A --alignment --resynthesis --align_notes --dynamics [--dynamics_rounds K] [--min_level_db L] --tuning auto|CENTS] [--key=value ...]``.

PATH is a state_dict file or a checkpoint directory holding transcription.ckpt; trailing ``--key=value`` pairs override keys of the yaml, as with
pretrain.py and finetune.py.  Writes DIR/NAME.json per recording (piano_a2s_amd/transcribe.py; --track_downbeats: piano_a2s_amd/beats.py, section 22);
with --resynthesis (it needs the downbeats) also DIR/NAME.resynth.wav, the recording beside the decoded score played back, and an agreement per bar
(piano_a2s_amd/resynth.py, section 24); with --align_notes (it implies --resynthesis) also every bar's notes where they are heard and DIR/NAME.mid,
the performed notes as a Standard MIDI File (section 25); with --dynamics (it implies --resynthesis) every note's level and velocity, estimated from
the recording by analysis by synthesis: the resynthesis is played at those dynamics and DIR/NAME.mid carries the velocities (section 26); with
--tuning auto the recording's tuning against A4 = 440 Hz is estimated and the features are shifted back onto the grid before the model sees them
(--tuning CENTS: by a known amount; piano_a2s_amd/tuning.py, section 27)."""
import sys

from piano_a2s_amd.transcribe import main

if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
