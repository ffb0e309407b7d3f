"""The multi-hand tracker on the CPU interpreter: the claim rule of a detect step's mask growth bit for bit against its
NumPy restatement (tests/helpers/track_hands_oracle.py) in both kernel forms, the per-slot box rule, the C surface's errors, and the
step executor at B = 1, K = 2 on a 32 x 32 frame -- seeded tracked steps without HandSegNet weights against the chain of per-op calls,
and a lost slot followed by a claimed detect step.  The interpreter needs about a minute per slot and step, so longer sequences are
marked slow (HP3D_SLOW=1); tests/test_gpu_track_hands.py runs the same helpers on the GPU at the shipped shapes."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth
from oracle import general as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO            # noqa: E402
import track_oracle as TO            # noqa: E402
import track_hands_oracle as THO     # noqa: E402

F32 = np.float32
skip_unless_slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="minutes per step on the CPU interpreter; set HP3D_SLOW=1")


def test_claim_rule_engineered_cases(emu_engine):
    THO.run_claim_cases(emu_engine)


def test_claim_rule_random_rectangles_with_random_keeps(emu_engine):
    THO.run_random_keeps(emu_engine, trials=6)


def test_claim_rule_nan_and_degenerate_boxes(emu_engine):
    """A comparison with a NaN is false: a kept slot whose box is not finite claims nothing; scale 0 gives half = inf and claims every
    object with a finite centre distance -- both as the restatement computes them in float32."""
    sm = HO.rect_scoremap(THO.RECTS5)
    for box in ((np.nan, 20.0, 2.0), (20.0, 20.0, np.nan), (np.inf, 20.0, 2.0), (20.0, 20.0, 0.0), (20.0, 20.0, np.inf)):
        got = THO.assert_keep_exact(emu_engine, sm, 2, THO.as_keep(2, {0: box}), both_forms=False)
        if box[2] == 0.0:
            assert got['claimed'][0, 0] == 5 and not got['valid'].any()
        elif not np.all(np.isfinite(box[:2])) or np.isnan(box[2]):
            assert got['claimed'][0, 0] == 0 and got['valid'][0].tolist() == [0, 1]


def test_per_slot_box_rule(emu_engine):
    rng = np.random.default_rng(21)
    for (B, K, H, W) in ((2, 3, 240, 320), (1, 4, 1080, 1920), (3, 1, 37, 53)):
        kp = rng.normal([H / 2, W / 2], [H / 2, W / 2], (B, K, 21, 2))
        kp[0, 0, 12] = np.nan
        valid = (rng.random((B, K)) < 0.6).astype(np.int32)
        valid[0, 0] = 1
        valid[-1, -1] = 0
        bc = rng.uniform(0, [H, W], (B, K, 2)).astype(F32)
        bs = rng.uniform(1, 5, (B, K)).astype(F32)
        sm = rng.standard_normal((B, K, 32, 32, 21)).astype(F32)
        c, s, conf, lost = THO.assert_box_slots(emu_engine, kp, valid, bc, bs, H, W, score32=sm)
        assert lost[0, 0] == 1 and lost[-1, -1] == 0
        THO.assert_box_slots(emu_engine, kp, valid, bc, bs, H, W)
        THO.assert_box_slots(emu_engine, kp, np.ones((B, K), np.int32), bc, bs, H, W)


def test_track_hands_errors_are_loud(emu_engine, synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        lib, h = e.lib, e.h
        img, hs = synth.make_batch(0, 1, 32, 48), HO.hand_sides(1, 2)
        c, s, v = np.array([[[16.0, 24.0], [10.0, 10.0]]], F32), np.array([[2.0, 3.0]], F32), np.array([[1, 1]], np.int32)
        with pytest.raises(_lib.Hp3dError, match="weights not finalized"):
            e.track_hands_step(img, hs, 2)
        nul = [None] * 13
        for K in (0, 5):
            assert lib.hp3d_track_hands_step(h, 1, 32, 48, K, _lib._ptr(img), _lib._ptr(hs), *nul) == -1
            assert "max hands" in lib.hp3d_last_error(h).decode()
            assert lib.hp3d_track_hands_step_dev(h, 1, 32, 48, K, _lib._ptr(img), _lib._ptr(hs), *nul) == -1
            assert lib.hp3d_track_hands_step_u8(h, 1, 32, 48, _lib._ptr(img), 32, 48, K, _lib._ptr(hs), *nul) == -1
            assert lib.hp3d_track_hands_seed(h, 1, 32, 48, K, _lib._ptr(c), _lib._ptr(s), _lib._ptr(v)) == -1
            assert "max hands" in lib.hp3d_last_error(h).decode()
            with pytest.raises(AssertionError, match="max hands"):
                e.masks_from_scoremap(synth.blob_scoremap('one_blob'), K, keep=(np.zeros((1, K), np.int32), np.zeros((1, K, 2), F32), np.ones((1, K), F32)))
        assert lib.hp3d_track_hands_step(h, 1, 32, 48, 2, None, _lib._ptr(hs), *nul) == -1
        assert lib.hp3d_track_hands_step(h, 1, 32, 48, 2, _lib._ptr(img), None, *nul) == -1
        assert "hand_side is NULL" in lib.hp3d_last_error(h).decode()
        assert lib.hp3d_track_hands_step_dev(h, 1, 32, 48, 2, None, None, *nul) == -1
        assert lib.hp3d_track_hands_step_u8(h, 1, 32, 48, None, 32, 48, 2, _lib._ptr(hs), *nul) == -1
        assert lib.hp3d_track_hands_seed(h, 1, 32, 48, 2, None, None, None) == -1
        assert lib.hp3d_track_hands_box(h, 1, 2, 32, 48, None, None, 0.0, *[None] * 7) == -1
        sm = synth.blob_scoremap('one_blob')
        assert lib.hp3d_masks_from_scoremap_keep(h, _lib._ptr(sm), 1, 120, 160, 2, None, None, None, *[None] * 8) == -1
        assert lib.hp3d_masks_from_scoremap_keep(h, None, 1, 120, 160, 2, _lib._ptr(v), _lib._ptr(c), _lib._ptr(s), *[None] * 8) == -1
        assert lib.hp3d_track_hands_reset(None) == -1 and lib.hp3d_track_hands_step(None, 1, 32, 48, 2, None, None, *nul) == -1
        with pytest.raises(NotImplementedError, match="must have the network size"):
            e.track_hands_step_u8(np.zeros((1, 64, 96, 3), np.uint8), hs, 2, H=32, W=48)
        # seeds: a bad scale or centre in a valid slot; the same values in an invalid slot are not looked at; no valid slot in an image
        for bad in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(AssertionError, match="positive and finite"):
                e.track_hands_seed(c, np.array([[2.0, bad]], F32), v, 32, 48)
            e.track_hands_seed(c, np.array([[2.0, bad]], F32), np.array([[1, 0]], np.int32), 32, 48)
        with pytest.raises(AssertionError, match="not finite"):
            e.track_hands_seed(np.array([[[np.nan, 1.0], [1.0, 1.0]]], F32), s, v, 32, 48)
        with pytest.raises(AssertionError, match="no valid slot"):
            e.track_hands_seed(np.tile(c, (2, 1, 1)), np.tile(s, (2, 1)), np.array([[1, 1], [0, 0]], np.int32), 32, 48)
        e.track_hands_reset()
        # PoseNet2D + lifting weights only: a detect step names the missing net (tracked steps run without it, below)
        e.load_weight_dict({k: w for k, w in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        with pytest.raises(_lib.Hp3dError, match="required network weights not loaded"):
            e.track_hands_step(img, hs, 2)
        assert e.counter('track_hands_detect_steps') == 0 and e.counter('track_hands_tracked_steps') == 0
    finally:
        e.close()
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: w for k, w in synth_weights.items() if k.startswith(('HandSegNet', 'PoseNet2D'))})
        e.finalize_weights(0)
        with pytest.raises(_lib.Hp3dError, match="required network weights not loaded"):
            e.track_hands_step(synth.make_batch(0, 1, 32, 48), HO.hand_sides(1, 2), 2)
    finally:
        e.close()


def test_python_surface():
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork
    assert hasattr(ColorHandPose3DNetwork, 'track_hands')


def test_seeded_tracked_steps_need_no_handsegnet(emu_engine, synth_weights):
    """PoseNet2D + lifting weights only, B = 1, K = 2, 32 x 32: both slots seeded at the frame's centre with scale 10, so every keypoint
    lands within 12.8 pixels of (16, 16), inside the frame: nothing is lost and the second step is a tracked one as well, cropping
    with the boxes track_box derives from the first step's keypoints.  The first step equals the chain of per-op calls at batch 2."""
    from hand3d_amd import _lib
    H = W = 32
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        assert e.nets_mask() & 1 == 0
        hs = HO.hand_sides(1, 2)
        center, scale, valid = np.full((1, 2, 2), 16.0, F32), np.full((1, 2), 10.0, F32), np.ones((1, 2), np.int32)
        e.track_hands_seed(center, scale, valid, H, W)
        m = THO.Machine()
        m.seed(center, scale, valid, H, W)
        o1, detect = THO.step_and_check(e, m, TO.frames(2, 0, 1, H, W), hs, 2)
        assert not detect and (e.counter('track_hands_detect_steps'), e.counter('track_hands_tracked_steps')) == (0, 1)
        assert not o1['lost'].any() and not o1['detected'].any() and np.all(o1['valid'] == 1)
        assert np.array_equal(o1['center'], center) and np.array_equal(o1['scale'], scale)
        f1 = TO.frames(2, 1, 1, H, W)
        o2 = e.track_hands_step(f1, hs, 2)
        assert (e.counter('track_hands_detect_steps'), e.counter('track_hands_tracked_steps')) == (0, 2)
        c, s, _, _ = e.track_box(o1['kp_hw'][0], H, W)
        assert np.array_equal(o2['center'][0], c) and np.array_equal(o2['scale'][0], s) and not o2['detected'].any()
        assert np.array_equal(o2['crop'][0], G.crop_image_from_xy(np.repeat(f1, 2, axis=0), c, 256, s))
    finally:
        e.close()


@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


def test_lost_slot_then_a_claimed_detect_step(net_engine):
    """B = 1, K = 2, 32 x 32, all weights: slot 1 seeded far outside the frame.  The first step is tracked and reports lost = [0, 1]; the
    next one is a detect step whose boxes, valid, detected, area and claimed are what the restatement gives on e.handsegnet(frame)
    with slot 0 kept."""
    e = net_engine
    H = W = 32
    hs = HO.hand_sides(1, 2)
    center = np.array([[[16.0, 16.0], [-5000.0, -7000.0]]], F32)
    scale, valid = np.array([[10.0, 1.0]], F32), np.ones((1, 2), np.int32)
    e.track_hands_seed(center, scale, valid, H, W)
    m = THO.Machine()
    m.seed(center, scale, valid, H, W)
    o1, detect = THO.step_and_check(e, m, TO.frames(4, 0, 1, H, W), hs, 2, want_kpmap=False, compose=False)
    assert not detect and o1['lost'][0].tolist() == [0, 1] and not o1['crop'][0, 1].any()
    f1 = TO.frames(4, 1, 1, H, W)
    n = e.counter('mask_grow_multi_launches')
    o2, detect = THO.step_and_check(e, m, f1, hs, 2, want_kpmap=False, compose=False)
    assert detect and e.counter('mask_grow_multi_launches') == n + 1
    assert o2['detected'][0, 0] == 0 and o2['valid'][0, 0] == 1
    c, s, _, _ = e.track_box(o1['kp_hw'][0, :1], H, W)
    assert np.array_equal(o2['center'][0, 0], c[0]) and o2['scale'][0, 0] == s[0]          # slot 0 kept its tracked box
    e.track_hands_reset()


@pytest.mark.slow
@skip_unless_slow
def test_three_steps_two_slots(net_engine, synth_weights):
    assert THO.run_steps(net_engine, synth_weights, 2, 2, 48, 64) >= 1
