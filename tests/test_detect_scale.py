"""Detection on a reduced frame (option "detect_scale") on the CPU interpreter: the two downscale kernels and the two box
maps bit for bit against tests/helpers/detect_scale_oracle.py, f = 1 changing nothing, one detect step at f = 2 as the composition of
the engine's own per-op calls, the claim rule at f = 2, and the errors.  The whole-step tests run at B = 1 on a 32 x 32 frame (a
16 x 16 detection frame at f = 2), like tests/test_track.py's; tests/test_gpu_detect_scale.py runs the shipped shapes on the GPU."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import detect_scale_oracle as DS      # noqa: E402
import track_oracle as TO             # noqa: E402

F32 = np.float32


@pytest.mark.parametrize("B,H,W,f", DS.DOWNSCALE_SHAPES + DS.DOWNSCALE_SHAPES_WIDE)
def test_downscale_bit_exact(emu_engine, B, H, W, f):
    DS.assert_downscale_exact(emu_engine, B, H, W, f)


def test_downscale_windows():
    """The helper itself on a case worked by hand: a 3 x 5 frame at f = 2 has windows of 4, 4, 2 / 2, 2, 1 pixels."""
    x = np.arange(15, dtype=F32).reshape(1, 3, 5, 1).repeat(3, axis=3)
    d = DS.downscale(x, 2)
    assert d.shape == (1, 2, 3, 3)
    assert d[0, :, :, 0].tolist() == [[(0 + 1 + 5 + 6) / 4, (2 + 3 + 7 + 8) / 4, (4 + 9) / 2], [(10 + 11) / 2, (12 + 13) / 2, 14.0]]
    u = DS.downscale_u8(x.astype(np.uint8), 2)
    assert np.array_equal(u, (d / F32(255) - F32(0.5)).astype(F32))
    assert DS.detect_shape(1080, 1920, 4) == (270, 480) and DS.detect_shape(33, 130, 8) == (5, 17)


@pytest.mark.parametrize("f", [2, 3, 4, 8])
def test_boxes_bit_exact(emu_engine, f):
    DS.assert_boxes_exact(emu_engine, f)


def test_claim_rule_at_f2(emu_engine):
    DS.run_claim_at(emu_engine, 2)


def test_errors_are_loud(emu_engine):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        for bad in ('0', '9', 'x', '', '2.0', '-1', '10'):
            with pytest.raises(AssertionError, match="detect_scale"):
                e.set_option('detect_scale', bad)
        lib, h = e.lib, e.h
        assert lib.hp3d_downscale(h, None, 1, 32, 32, 2, None) == -1 and lib.hp3d_downscale_u8(h, None, 1, 32, 32, 2, None) == -1
        assert lib.hp3d_boxes_to_frame(h, 1, 2, None, None, None, None, None) == -1
        assert lib.hp3d_boxes_to_detect(h, 1, 2, None, None, None, None) == -1
        with pytest.raises(AssertionError):
            e.downscale(np.zeros((1, 32, 32, 3), F32), 9)
        # a 24 x 24 frame at f = 2 has a 12 x 12 detection frame: refused before anything is looked at or launched (this context has
        # no weights at all, and the refusal is about the argument), by every entry point the option applies to; f = 1 gets as far as
        # the missing weights
        e.set_option('detect_scale', '2')
        img, hs = synth.make_batch(0, 1, 24, 24), synth.hand_sides(1)
        n0 = {k: e.counter(k) for k in DS.COUNTERS}
        e.set_profiling(1)
        for step in (lambda: e.track_step(img, hs), lambda: e.track_step_u8(TO.to_u8(img), hs),
                     lambda: e.track_hands_step(img, hs.reshape(1, 1, 2), 1), lambda: e.track_hands_step_u8(TO.to_u8(img), hs.reshape(1, 1, 2), 1)):
            with pytest.raises(AssertionError, match="detection frame"):
                step()
        assert {k: e.counter(k) for k in DS.COUNTERS} == n0 and not e.profile()
        e.set_profiling(0)
        with pytest.raises(_lib.Hp3dError, match="weights not finalized"):
            e.track_step(synth.make_batch(0, 1, 32, 32), hs)          # 16 x 16: accepted
        e.set_option('detect_scale', '1')
        with pytest.raises(_lib.Hp3dError, match="weights not finalized"):
            e.track_step(img, hs)
    finally:
        e.close()


@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


def test_f1_changes_nothing(net_engine):
    """One detect step of track_step at B = 1 on a 32 x 32 frame with the option unset (a fresh context's default) and set to "1": the
    same outputs, profile rows and counters."""
    from hand3d_amd import _lib
    e = net_engine
    fr, hs = TO.frames(4, 1, 1, 32, 32), synth.hand_sides(1)
    e.set_option('detect_scale', '1')
    e.track_reset()
    o1, rows1, dn1 = DS.run_detect_step(e, lambda: e.track_step(fr, hs, want_kpmap=True))
    e.track_reset()
    unset = _lib.Engine(0, path=e.lib._name)          # never saw the option
    try:
        unset.load_weight_dict(synth.make_weights())
        unset.finalize_weights(0)
        o0, rows0, dn0 = DS.run_detect_step(unset, lambda: unset.track_step(fr, hs, want_kpmap=True))
    finally:
        unset.close()
    assert rows0 == rows1 and dn0 == dn1
    assert dn1['track_detect_steps'] == 1 and dn1['detect_scale_steps'] == 0
    assert not [r for r in rows1 if r.startswith(('downscale', 'box_to'))] and 'mask_grow' in rows1 and 'track_select' in rows1
    for k, v in o0.items():
        assert np.array_equal(v, o1[k]), k


def test_detect_step_at_f2_is_the_composition(net_engine):
    """B = 1, 32 x 32, f = 2: center, scale_crop and image_crop of a detect step equal downscale -> handsegnet at (16, 16) ->
    mask_from_scoremap -> rule 3 -> crop_and_resize on the full frame, bit for bit.  (One step: PoseNet2D on the interpreter takes
    over a minute.  That a change of the option makes the next step detect is held on the GPU, tests/test_gpu_detect_scale.py.)"""
    e = net_engine
    fr, hs = TO.frames(4, 1, 1, 32, 32), synth.hand_sides(1)
    e.track_reset()
    e.set_option('detect_scale', '2')
    try:
        o, rows, dn = DS.run_detect_step(e, lambda: e.track_step(fr, hs))
        assert (dn['track_detect_steps'], dn['detect_scale_steps'], dn['crop_u8_launches']) == (1, 1, 0)
        DS.assert_detect_step_is_composition(e, o, rows, fr, 2)
    finally:
        e.set_option('detect_scale', '1')
        e.track_reset()
