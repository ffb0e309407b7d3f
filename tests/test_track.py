"""Tracking on the CPU interpreter: the box rule and the uint8 crop bit for bit, the C surface's errors, and the step
executor at B = 1 on a 32 x 32 frame (seeded tracked steps without HandSegNet weights against the chain of existing ops; a lost hand
followed by a detect step).  The interpreter needs over a minute per image and step, so the three-step and seed / loss /
re-detection checks at B = 2 (tests/helpers/track_oracle.py) are marked slow and run with HP3D_SLOW=1, like the other whole-path
interpreter test; tests/test_gpu_track.py runs the same helpers on the GPU at the shipped shapes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth
from hand3d_amd.data.BinaryDbReader import _gt_hand_crop
from oracle import general as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import track_oracle as TO      # noqa: E402

F32 = np.float32
skip_unless_slow = pytest.mark.skipif(os.environ.get('HP3D_SLOW') != '1', reason="minutes per step on the CPU interpreter; set HP3D_SLOW=1")


def box_cases(H, W, rng):
    """Random keypoint sets plus engineered ones; [n,21,2] float64 (row, col)."""
    cases = [rng.uniform(0, [H, W], (21, 2)) for _ in range(24)]
    cases += [rng.normal([H / 2, W / 2], [H, W], (21, 2)) for _ in range(24)]          # many outside the frame
    mid = np.array([H / 2.0, W / 2.0])
    k = rng.uniform(0, [H, W], (21, 2)); k[12] = np.nan; cases.append(k)                # keypoint 12 NaN: centre (0, 0)
    k = rng.uniform(0, [H, W], (21, 2)); k[12, 1] = np.inf; cases.append(k)
    cases.append(np.tile(mid, (21, 1)))                                                 # all equal: size 50, scale 256 / 50
    k = np.tile(mid, (21, 1)); k[0] = mid + [300.0, 0.0]; k[1] = mid - [300.0, 0.0]; cases.append(k)      # spread beyond 500 (frame permitting)
    k = np.tile(mid, (21, 1)); k[0] = mid + [0.0, 1.0]; cases.append(k)                 # scale clamp 10 (size 50 -> 5.12; tiny boxes stay there)
    k = np.tile(mid, (21, 1)); k[0] = mid + [180.0, 0.0]; cases.append(k)               # size 360: scale clamps to 1
    for side in range(4):                                                               # keypoints outside the frame on each side
        k = rng.uniform(0.25, 0.75, (21, 2)) * [H, W]
        k[3 + side] = [(-40.0, W / 2), (H + 40.0, W / 2), (H / 2, -40.0), (H / 2, W + 40.0)][side]
        cases.append(k)
        k = k.copy(); k[12] = k[3 + side]; cases.append(k)                              # ... and the centre itself: lost
    cases.append(np.full((21, 2), np.nan))                                              # all NaN: size 200
    return np.stack(cases).astype(np.float64)


@pytest.mark.parametrize("H,W", [(240, 320), (1080, 1920), (37, 53)])
def test_track_box_is_the_readers_rule(emu_engine, H, W):
    rng = np.random.default_rng(H)
    kp = box_cases(H, W, rng)
    for margin in (1.0, 1.25):
        c, s, conf, lost = emu_engine.track_box(kp, H, W, margin=margin)
        rc, rs, rl = TO.box_rule_batch(kp, H, W, margin)
        assert np.array_equal(c, rc) and np.array_equal(s, rs) and np.array_equal(lost, rl), margin
        assert np.all(conf == 0)
    # the engineered expectations themselves (margin 1)
    c, s, _, lost = emu_engine.track_box(kp, H, W, margin=1)
    n = 48
    assert np.array_equal(c[n], [0, 0]) and lost[n] == 1 and lost[n + 1] == 1
    assert s[n + 2] == F32(256) / F32(50) and lost[n + 2] == 0
    if H >= 700:
        assert s[n + 3] == F32(1) and TO.box_rule(kp[n + 3], H, W)[1] == F32(1)
    assert s[n + 5] == F32(1) if H >= 400 else True
    assert s[-1] == F32(256) / F32(200) and lost[-1] == 1 and np.array_equal(c[-1], [0, 0])
    assert lost.sum() == sum(1 for k in kp if not np.all(np.isfinite(k[12])) or k[12, 0] < 0 or k[12, 0] > H or k[12, 1] < 0 or k[12, 1] > W)
    assert 0 < lost.sum() < len(lost)
    # default option = 1.25, and the Python margin= argument leaves it alone
    assert np.array_equal(emu_engine.track_box(kp, H, W)[1], TO.box_rule_batch(kp, H, W, 1.25)[1])


def test_track_box_equals_gt_hand_crop(emu_engine):
    """margin 1 == what the reader computes from ground-truth keypoints (crop_scale; the centre through its crop)."""
    H, W = 48, 64
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    kps = list(rng.uniform(-10, [H + 10, W + 10], (6, 21, 2)))
    k = kps[0].copy(); k[12] = np.nan; kps.append(k)
    for kp in kps:
        uv = kp[:, ::-1].astype(F32)
        d = {'keypoint_uv21': uv.copy(), 'keypoint_vis21': np.ones(21, bool), 'cam_mat': np.eye(3, dtype=F32)}
        _gt_hand_crop(d, img, (H, W), 256, emu_engine)
        c, s, _, _ = emu_engine.track_box(kp[None].astype(F32).astype(np.float64), H, W, margin=1)
        assert d['crop_scale'] == s[0]
        assert np.array_equal(d['image_crop'], emu_engine.crop_and_resize_u8(img[None], c, s, 256)[0])


def test_track_confidence_and_min_score(emu_engine):
    rng = np.random.default_rng(9)
    sm = rng.standard_normal((3, 32, 32, 21)).astype(F32)
    sm[1, 5, 5, 3] = np.nan
    kp = np.tile(np.array([100.0, 100.0]), (3, 21, 1))
    _, _, conf, lost = emu_engine.track_box(kp, 240, 320, score32=sm)
    assert np.array_equal(conf, TO.confidence(sm)) and not lost.any()
    emu_engine.set_option('track_min_score', repr(float(np.sort(conf)[1])))
    try:
        _, _, conf2, lost = emu_engine.track_box(kp, 240, 320, score32=sm)
        assert np.array_equal(lost, (conf < np.sort(conf)[1]).astype(np.int32)) and lost.sum() == 1
    finally:
        emu_engine.set_option('track_min_score', 'off')
    assert not emu_engine.track_box(kp, 240, 320, score32=sm)[3].any()


@pytest.mark.parametrize("B,H,W", [(3, 37, 53), (2, 240, 320), (1, 720, 1280)])
def test_crop_and_resize_u8_bit_exact(emu_engine, B, H, W):
    rng = np.random.default_rng(W)
    u8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    pre = emu_engine.preprocess_u8(u8, H, W)
    assert np.array_equal(pre, G.preprocess_u8(u8, H, W))
    boxes = [(rng.uniform(0, [H, W], (B, 2)), rng.uniform(1, 10, B)),                    # inside
             (rng.uniform(-0.3, 1.3, (B, 2)) * [H, W], rng.uniform(0.5, 4, B)),          # partly outside
             (np.tile([-3.0 * H, 5.0 * W], (B, 1)), np.full(B, 2.0)),                    # wholly outside
             (rng.uniform(0, [H, W], (B, 2)), np.full(B, 1.0)), (rng.uniform(0, [H, W], (B, 2)), np.full(B, 10.0))]     # the scale clamps
    n0 = emu_engine.counter('crop_u8_launches')
    for center, scale in boxes:
        center, scale = center.astype(F32), scale.astype(F32)
        got = emu_engine.crop_and_resize_u8(u8, center, scale, 64)
        assert np.array_equal(got, emu_engine.crop_and_resize(pre, center, scale, 64))
        assert np.array_equal(got, G.crop_image_from_xy(pre, center, 64, scale))
    assert emu_engine.counter('crop_u8_launches') == n0 + len(boxes)
    assert not boxes[2][0].size or np.all(emu_engine.crop_and_resize_u8(u8, boxes[2][0].astype(F32), boxes[2][1].astype(F32), 16) == 0)


def test_track_errors_are_loud(emu_engine, synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        lib, h = e.lib, e.h
        img = synth.make_batch(0, 1, 32, 48)
        hs = synth.hand_sides(1)
        ok = np.array([[16.0, 24.0]], F32), np.array([2.0], F32)
        # no weights at all
        with pytest.raises(_lib.Hp3dError, match="weights not finalized"):
            e.track_step(img, hs)
        # NULL pointers
        nul = [None] * 10
        assert lib.hp3d_track_step(h, 1, 32, 48, None, _lib._ptr(hs), *nul) == -1
        assert lib.hp3d_track_step(h, 1, 32, 48, _lib._ptr(img), None, *nul) == -1
        assert lib.hp3d_track_step_dev(h, 1, 32, 48, None, None, *nul) == -1
        assert lib.hp3d_track_step_u8(h, 1, 32, 48, None, 32, 48, _lib._ptr(hs), *nul) == -1
        assert lib.hp3d_track_seed(h, 1, 32, 48, None, None) == -1
        assert lib.hp3d_track_box(h, 1, 32, 48, None, None, 0.0, None, None, None, None) == -1
        assert lib.hp3d_crop_and_resize_u8(h, None, 1, 32, 48, None, None, 8, None) == -1
        assert lib.hp3d_track_reset(None) == -1 and lib.hp3d_track_step(None, 1, 32, 48, None, None, *nul) == -1
        # uint8 frame of another size than the network's
        with pytest.raises(NotImplementedError, match="must have the network size"):
            e.track_step_u8(np.zeros((1, 64, 96, 3), np.uint8), hs, H=32, W=48)
        # seeds
        for bad in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(AssertionError, match="positive and finite"):
                e.track_seed(ok[0], np.array([bad], F32), 32, 48)
        with pytest.raises(AssertionError, match="not finite"):
            e.track_seed(np.array([[np.nan, 1.0]], F32), ok[1], 32, 48)
        for k, v in (('track_margin', '0'), ('track_margin', 'x'), ('track_min_score', 'nan'), ('track_redetect', '-1')):
            with pytest.raises(AssertionError):
                e.set_option(k, v)
        # PoseNet2D + lifting weights only: a detect step names the missing net ...
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        assert e.nets_mask() & 1 == 0
        with pytest.raises(_lib.Hp3dError, match="required network weights not loaded"):
            e.track_step(img, hs)
        assert e.counter('track_detect_steps') == 0 and e.counter('track_tracked_steps') == 0
        # (... and tracked steps run without it: test_seeded_tracked_steps_need_no_handsegnet)
    finally:
        e.close()
    # lifting weights missing
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if k.startswith(('HandSegNet', 'PoseNet2D'))})
        e.finalize_weights(0)
        with pytest.raises(_lib.Hp3dError, match="required network weights not loaded"):
            e.track_step(synth.make_batch(0, 1, 32, 48), synth.hand_sides(1))
    finally:
        e.close()


@pytest.fixture(scope='module')
def net_engine(emu_engine, synth_weights):
    emu_engine.load_weight_dict(synth_weights)
    emu_engine.finalize_weights(0)
    return emu_engine


def test_seeded_tracked_steps_need_no_handsegnet(emu_engine, synth_weights):
    """PoseNet2D + lifting weights only, B = 1, 32 x 32: track_seed -> two tracked steps.  Seeded at the frame's centre with scale 10
    the crop spans 25.6 pixels, so every keypoint lands within 12.8 pixels of (16, 16), inside the frame: nothing is lost and the
    second step must be a tracked one as well, cropping with the box the first step's keypoints give.  The first step equals the
    chain of existing ops bit for bit."""
    from hand3d_amd import _lib
    H = W = 32
    e = _lib.Engine(0, path=emu_engine.lib._name)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        assert e.nets_mask() & 1 == 0
        hs = synth.hand_sides(1)
        center, scale = np.array([[16.0, 16.0]], F32), np.array([10.0], F32)
        e.track_seed(center, scale, H, W)
        e.set_profiling(1)
        o1 = e.track_step(TO.frames(2, 0, 1, H, W), hs, want_kpmap=True)
        assert TO.no_seg_rows(e) and e.get_timing()['HandSegNet'] == 0.0
        assert [r[0] for r in e.profile() if r[0] in ('crop_and_resize', 'kp_detect', 'track_box')] == ['crop_and_resize', 'kp_detect', 'track_box']
        e.set_profiling(0)
        assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (0, 1)
        assert np.all(o1['detected'] == 0) and np.all(o1['lost'] == 0)
        TO.assert_step_is_composition(e, o1, TO.frames(2, 0, 1, H, W), hs, center, scale, H, W)
        o2 = e.track_step(TO.frames(2, 1, 1, H, W), hs)
        assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (0, 2)
        c, s, _, _ = e.track_box(o1['kp_hw'], H, W)
        assert np.array_equal(o2['center'], c) and np.array_equal(o2['scale'].reshape(-1), s) and np.all(o2['detected'] == 0)
        assert np.array_equal(o2['crop'], G.crop_image_from_xy(TO.frames(2, 1, 1, H, W), c, 256, s))
    finally:
        e.close()


def test_lost_hand_makes_the_next_step_detect(net_engine):
    """B = 1, 32 x 32, all weights: seeded far outside the frame, the tracked step reports the hand as lost; the step behind it is a
    detect step whose box is HandSegNet's (hp3d_handsegnet -> hp3d_mask_from_scoremap on the same frame), detected = 1."""
    e = net_engine
    H = W = 32
    hs = synth.hand_sides(1)
    e.track_seed(np.array([[-5000.0, -7000.0]], F32), np.array([1.0], F32), H, W)
    nd, nt = e.counter('track_detect_steps'), e.counter('track_tracked_steps')
    o1 = e.track_step(TO.frames(4, 0, 1, H, W), hs)
    assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (nd, nt + 1)
    assert o1['lost'][0] == 1 and o1['detected'][0] == 0 and not o1['crop'].any()
    f1 = TO.frames(4, 1, 1, H, W)
    e.set_profiling(1)
    o2 = e.track_step(f1, hs)
    rows = [r[0] for r in e.profile()]
    e.set_profiling(0)
    assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (nd + 1, nt + 1)
    assert 'track_select' in rows and 'mask_grow' in rows and e.counter('track_detect_steps') == nd + 1
    _, center, _, scale, _ = e.mask_from_scoremap(e.handsegnet(f1))
    assert o2['detected'][0] == 1 and np.array_equal(o2['center'], center) and np.array_equal(o2['scale'], scale)
    assert np.array_equal(o2['crop'], G.crop_image_from_xy(f1, center, 256, scale))
    e.track_reset()


@pytest.mark.slow
@skip_unless_slow
def test_tracked_steps_are_the_composition_and_match_the_oracle(net_engine, synth_weights):
    """B = 2 on a small frame, three steps: the first detects and equals infer_full + detect_keypoints, the others are tracked and equal
    the chain of existing ops and the oracle.  (On a frame this small random weights lose every hand, so lost images are re-seeded
    with the boxes their own keypoints give: reseed_lost.)"""
    assert TO.run_three_steps(net_engine, synth_weights, 2, 48, 64, reseed_lost=True) == 2


@pytest.mark.slow
@skip_unless_slow
def test_seed_loss_and_redetection(net_engine):
    TO.run_seed_loss_redetect(net_engine, 2, 48, 64)
