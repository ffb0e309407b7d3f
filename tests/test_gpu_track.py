"""Tracking through the real library: the uint8 crop bit for bit, a tracked step as the composition of the existing
ops (bit for bit: the same kernels at the same shapes) and against the oracle stage by stage, and the seed / loss / re-detection
rules -- at B = 1 240x320 (fused lifting stage), B = 8 and B = 32 at 320x320 (filled-launch kernel plan) and B = 1 uint8 at
720x1280 (global mask growth on the detect step, the uint8 crop on the tracked ones).  The checks live in
tests/helpers/track_oracle.py, shared with the interpreter tests."""
import os
import sys

import numpy as np
import pytest

from oracle import general as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import track_oracle as TO      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def eng(gpu_engine, synth_weights):
    gpu_engine.load_weight_dict(synth_weights)
    gpu_engine.finalize_weights(0)
    return gpu_engine


@pytest.mark.parametrize("B,H,W", [(3, 37, 53), (2, 240, 320), (1, 1080, 1920)])
def test_crop_and_resize_u8_bit_exact(gpu_engine, B, H, W):
    rng = np.random.default_rng(W)
    u8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    pre = gpu_engine.preprocess_u8(u8, H, W)
    boxes = [(rng.uniform(0, [H, W], (B, 2)), rng.uniform(1, 10, B)),
             (rng.uniform(-0.3, 1.3, (B, 2)) * [H, W], rng.uniform(0.5, 4, B)),
             (np.tile([-3.0 * H, 5.0 * W], (B, 1)), np.full(B, 2.0)),
             (rng.uniform(0, [H, W], (B, 2)), np.full(B, 1.0)), (rng.uniform(0, [H, W], (B, 2)), np.full(B, 10.0))]
    for center, scale in boxes:
        center, scale = center.astype(F32), scale.astype(F32)
        got = gpu_engine.crop_and_resize_u8(u8, center, scale, 256)
        assert np.array_equal(got, gpu_engine.crop_and_resize(pre, center, scale, 256))
        assert np.array_equal(got, G.crop_image_from_xy(pre, center, 256, scale))


def test_track_box_rule_on_device(gpu_engine):
    rng = np.random.default_rng(1)
    H, W = 240, 320
    kp = rng.normal([H / 2, W / 2], [H, W], (64, 21, 2))
    kp[5, 12] = np.nan
    kp[6] = np.nan
    sm = rng.standard_normal((64, 32, 32, 21)).astype(F32)
    for margin in (1.0, 1.25):
        c, s, conf, lost = gpu_engine.track_box(kp, H, W, score32=sm, margin=margin)
        rc, rs, rl = TO.box_rule_batch(kp, H, W, margin)
        assert np.array_equal(c, rc) and np.array_equal(s, rs) and np.array_equal(lost, rl)
        assert np.array_equal(conf, TO.confidence(sm))


@pytest.mark.parametrize("B,H,W,u8", [(1, 240, 320, False), (8, 320, 320, False), (32, 320, 320, False), (1, 720, 1280, True)])
def test_tracked_steps_are_the_composition_and_match_the_oracle(eng, synth_weights, B, H, W, u8):
    ng = eng.counter('mask_grow_global_launches')
    nf = eng.counter('lift_fused_launches')
    n = TO.run_three_steps(eng, synth_weights, B, H, W, seed=B + H, u8=u8, oracle_images=None if B <= 8 else (0, B // 2, B - 1),
                           reseed_lost=B > 8)
    print("B=%d %dx%d u8=%s: %d tracked steps of 2" % (B, H, W, u8, n))
    assert n >= 1, "no step was tracked: random-weight keypoints 12 left the frame in every step -- pick another seed"
    if u8:
        assert eng.counter('mask_grow_global_launches') > ng
    if B == 1:
        assert eng.counter('lift_fused_launches') > nf


def test_tracked_steps_half_precision_trunks(synth_weights):
    """Tracked steps as the chain of existing ops with hp3d_finalize_weights(ctx, 1): an engine of its own, as the other half-precision tests take one."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        hs = TO.synth.hand_sides(8)
        prev, ntracked = None, 0
        for t in range(3):
            fr = TO.frames(21, t, 8, 320, 320)
            nt = e.counter('track_tracked_steps')
            o = e.track_step(fr, hs, want_kpmap=True)
            if t > 0 and not prev['lost'].any():
                assert e.counter('track_tracked_steps') == nt + 1
                c, s, _, _ = e.track_box(prev['kp_hw'], 320, 320)
                TO.assert_step_is_composition(e, o, fr, hs, c, s, 320, 320)
                ntracked += 1
            prev = o
        assert ntracked >= 1, "pick another seed"
    finally:
        e.close()


@pytest.mark.parametrize("B,H,W", [(8, 320, 320), (32, 320, 320)])
def test_seed_loss_and_redetection(eng, B, H, W):
    kept = TO.run_seed_loss_redetect(eng, B, H, W)
    print("B=%d: %d images kept their tracked box through the detect step" % (B, kept))
    assert kept >= 1


def test_tracked_step_needs_no_handsegnet(synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict({k: v for k, v in synth_weights.items() if not k.startswith('HandSegNet')})
        e.finalize_weights(0)
        img, hs = TO.synth.make_batch(0, 2, 240, 320), TO.synth.hand_sides(2)
        with pytest.raises(_lib.Hp3dError, match="required network weights not loaded"):
            e.track_step(img, hs)
        e.track_seed(np.array([[120, 160], [100, 100]], F32), np.array([2.0, 3.0], F32), 240, 320)
        o = e.track_step(img, hs)
        assert e.counter('track_tracked_steps') == 1 and np.all(o['detected'] == 0) and np.isfinite(o['coord3d']).all()
    finally:
        e.close()


def test_track_step_dev_equals_host_step(eng):
    """The device-pointer entry point: same outputs as the host call, flags through the context's page-locked buffer."""
    B, H, W = 2, 240, 320
    hs = TO.synth.hand_sides(B)
    fr = [TO.frames(5, t, B, H, W) for t in range(3)]
    eng.track_reset()
    host = [eng.track_step(f, hs) for f in fr]
    eng.track_reset()
    d_hs = eng.to_device(hs)
    bufs = {k: eng.dev_alloc(n) for k, n in (('coord3d', B * 63 * 4), ('kp_hw', B * 42 * 8), ('center', B * 8), ('scale', B * 4),
                                             ('confidence', B * 4), ('lost', B * 4), ('detected', B * 4))}
    for t, f in enumerate(fr):
        d_img = eng.to_device(f)
        eng.track_step_dev(B, H, W, d_img, d_hs, **{k: int(v) for k, v in bufs.items()})
        eng.sync()
        for k, shape, dt in (('coord3d', (B, 21, 3), F32), ('kp_hw', (B, 21, 2), np.float64), ('center', (B, 2), F32),
                             ('scale', (B, 1), F32), ('confidence', (B,), F32), ('lost', (B,), np.int32), ('detected', (B,), np.int32)):
            assert np.array_equal(eng.to_host(bufs[k], shape, dt), host[t][k]), (t, k)
        d_img.free()
    eng.track_reset()
