"""Option "track_partial_detect"  on the CPU interpreter: the option's values, hp3d_gather_frames against the existing
per-ops bit for bit with its argument errors, and the step executor through tests/helpers/track_partial_oracle.py -- a detect step
that runs HandSegNet on the lost frames only, image by image against the same two steps on a second engine with the option off.  The
interpreter needs over a minute per image and step, so the step checks are marked slow and run with HP3D_SLOW=1 like
tests/test_track.py's; tests/test_gpu_track_partial.py runs the same helpers on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import track_partial_oracle as TP      # noqa: E402

skip_unless_slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="minutes per step on the CPU interpreter; set HP3D_SLOW=1")


def test_option_values(emu_engine):
    try:
        for v in ('0', '1'):
            emu_engine.set_option('track_partial_detect', v)
        for v in ('2', 'on', ''):
            with pytest.raises(AssertionError, match="track_partial_detect wants 0 or 1"):
                emu_engine.set_option('track_partial_detect', v)
    finally:
        emu_engine.set_option('track_partial_detect', '0')


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("f", [1, 2, 3])
@pytest.mark.parametrize("B,H,W", TP.GATHER_SHAPES)
def test_gather_frames_bit_exact(emu_engine, B, H, W, f, u8):
    n0 = emu_engine.counter('frame_gather_launches')
    for idx in TP.gather_indices(B):
        TP.assert_gather_frames_exact(emu_engine, B, H, W, f, idx, u8)
    assert emu_engine.counter('frame_gather_launches') - n0 == (4 if (f == 1 and not u8) else 0)


def test_gather_frames_errors(emu_engine):
    TP.assert_gather_frames_errors(emu_engine)


@pytest.fixture(scope='module')
def engines(emu_engine, synth_weights):
    from hand3d_amd import _lib
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    off = _lib.Engine(0, path=emu_engine.lib._name)
    off.load_weight_dict(synth_weights)
    off.finalize_weights(0)
    yield emu_engine, off
    off.close()
    emu_engine.track_reset()


@pytest.mark.slow
@skip_unless_slow
def test_partial_step_b3_32x32(engines):
    """B = 3, 32 x 32, lost = {1}: HandSegNet at batch 1; image 1's box is infer_full's on frame 1 alone, images 0 and 2 are bit-equal in
    every output to the option-off run."""
    o2 = TP.assert_partial_step(engines[0], engines[1], 3, 32, 32, [1], False, 1)
    assert o2['detected'].tolist() == [0, 1, 0]


@pytest.mark.slow
@skip_unless_slow
def test_partial_step_u8(engines):
    TP.assert_partial_step(engines[0], engines[1], 3, 32, 32, [1], True, 1)


@pytest.mark.slow
@skip_unless_slow
def test_partial_step_f2_64x64(engines):
    TP.assert_partial_step(engines[0], engines[1], 3, 64, 64, [1], False, 2)


@pytest.mark.slow
@skip_unless_slow
def test_partial_step_chunks(engines):
    """micro_batch = 2, B = 5, lost = {1, 4}: chunk 0 is partial (m = 1), chunk 1 is enqueued as a tracked chunk, chunk 2 (one frame,
    lost) takes the whole-chunk path; one detect step."""
    o2 = TP.assert_partial_step(engines[0], engines[1], 5, 32, 32, [1, 4], False, 1, micro_batch=2)
    assert o2['detected'].tolist() == [0, 1, 0, 0, 1]


@pytest.mark.slow
@skip_unless_slow
def test_fresh_and_scheduled_steps_untouched(engines):
    TP.assert_scheduled_and_fresh_untouched(engines[0], 32, 32)


@pytest.mark.slow
@skip_unless_slow
def test_other_entry_points_ignore_the_option(engines):
    TP.assert_other_entry_points_ignore(engines[0], 32, 32)
