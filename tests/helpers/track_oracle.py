"""NumPy restatement of the tracking box rule and the checks the CPU (interpreter) and GPU tracking tests share.

The rule is the dataset readers' hand_crop (data/BinaryDbReader.py:268-308 of the reference; hand3d_amd/data/BinaryDbReader.py:
_gt_hand_crop here) with all 21 keypoints visible and a margin factor on the size; see DESIGN.md 4.11."""
import numpy as np

from hand3d_amd import synth
from hand3d_amd.utils import general as PG
from oracle import general as G
from oracle import nets as N
from oracle import tf_ops as T

F32 = np.float32
TOL_HEATMAP = 1e-3          # the project's full-path gates
TOL_KP3D = 1e-4


def box_rule(kp_hw, H, W, margin=1.0, crop=256):
    """One image: keypoints [21,2] (row, col) -> (center [2] f32, scale f32, lost bool)."""
    kp = np.asarray(kp_hw, np.float64).astype(F32)
    c12 = kp[12]
    fin = bool(np.all(np.isfinite(c12)))
    center = c12 if fin else np.array([0.0, 0.0], F32)
    with np.errstate(invalid='ignore', over='ignore'):
        mn = np.maximum(kp.min(0), F32(0.0))
        mx = np.minimum(kp.max(0), np.array([H, W], F32))
        best = F32(2) * np.maximum(mx - center, center - mn)
        best = F32(best.max() * F32(margin))
        best = np.minimum(np.maximum(best, F32(50.0)), F32(500.0))
    if not np.isfinite(best):
        best = F32(200.0)
    scale = np.minimum(np.maximum(F32(crop) / best, F32(1.0)), F32(10.0)).astype(F32)
    lost = (not fin) or bool(c12[0] < 0 or c12[0] > F32(H) or c12[1] < 0 or c12[1] > F32(W))
    return center.astype(F32), scale, lost


def box_rule_batch(kp_hw, H, W, margin=1.0):
    r = [box_rule(k, H, W, margin) for k in kp_hw]
    return (np.stack([x[0] for x in r]), np.array([x[1] for x in r], F32), np.array([x[2] for x in r], np.int32))


def confidence(sm32):
    """[B,32,32,21] -> [B]: per channel the maximum (NaNs never win), added in channel order in float32, / 21."""
    m = np.where(np.isnan(sm32), -np.inf, sm32).astype(F32).max(axis=(1, 2))
    out = np.zeros(sm32.shape[0], F32)
    for b in range(sm32.shape[0]):
        s = F32(0.0)
        for c in range(21):
            s = F32(s + m[b, c])
        out[b] = F32(s / F32(21.0))
    return out


def frames(seed, t, B, H, W):
    return synth.make_batch(seed + 100 * t, B, H, W)


def to_u8(img):
    return np.clip(np.rint((img + 0.5) * 255.0), 0, 255).astype(np.uint8)


def no_seg_rows(engine):
    return not [r for r in engine.profile() if r[0].startswith('HandSegNet/') or r[0] in ('seg_upsample_softmax', 'mask_grow')]


def compose(e, frame, hs, center, scale):
    """The chain of existing ops a step's back half is made of, on the same engine."""
    crop = e.crop_and_resize(frame, center, scale, 256)
    sm = e.posenet2d(crop)[2]
    coord3d = e.pose3d(sm, hs)[0]
    kp_crop = e.detect_keypoints(sm)
    kp_hw = np.stack([PG.trafo_coords(kp_crop[b], center[b:b + 1], scale[b:b + 1].reshape(1, 1), 256) for b in range(len(kp_crop))])
    kpmap = e.resize_bilinear(sm, 256, 256)
    return {'crop': crop, 'sm': sm, 'coord3d': coord3d, 'kp_crop': kp_crop, 'kp_hw': kp_hw, 'kpmap': kpmap}


def assert_step_is_composition(e, o, frame, hs, center, scale, H, W):
    """Every output of step `o` equals the chain of existing ops at the boxes (center, scale)."""
    assert np.array_equal(o['center'], center) and np.array_equal(o['scale'].reshape(-1), scale.reshape(-1))
    c = compose(e, frame, hs, o['center'], o['scale'].reshape(-1))
    assert np.array_equal(o['crop'], c['crop'])
    for k in ('kpmap', 'coord3d', 'kp_crop', 'kp_hw'):
        if o[k] is None:
            continue
        assert np.array_equal(o[k], c[k]), k          # the same kernels at the same shapes: no tolerance
    nc, ns, conf, lost = e.track_box(o['kp_hw'], H, W, score32=c['sm'])
    assert np.array_equal(o['confidence'], conf)
    assert np.array_equal(o['lost'], lost)
    assert np.array_equal(lost, box_rule_batch(o['kp_hw'], H, W, 1.25)[2])
    assert np.array_equal(conf, confidence(c['sm']))
    return nc, ns


def assert_step_vs_oracle(o, frame, hs, weights, images):
    """Stage-wise against the oracle on the device's own box / crop (DESIGN.md 2 gates)."""
    assert np.array_equal(o['crop'], G.crop_image_from_xy(frame, o['center'], 256, o['scale']))
    for b in images:
        sm32 = N.posenet2d(weights, o['crop'][b:b + 1])[-1]
        assert np.abs(o['kpmap'][b:b + 1] - T.resize_bilinear_legacy(sm32, 256, 256)).max() < TOL_HEATMAP, b
        assert np.abs(o['coord3d'][b:b + 1] - N.pose3d(weights, sm32, hs[b:b + 1])[0]).max() < TOL_KP3D, b


def run_three_steps(e, weights, B, H, W, seed=7, u8=False, oracle_images=None, reseed_lost=False):
    """Three steps: step 0 detects and equals infer_full + detect_keypoints; a later step is tracked -- no HandSegNet rows,
    equal to the chain of existing ops fed from the device's previous keypoints, and to the oracle stage by stage -- unless the step
    before it flagged an image as lost (random weights put keypoint 12 anywhere in the crop): then it detects, and the lost images
    take infer_full's box while the others keep the tracked one.  reseed_lost (large batches, where some random-weight image is
    lost in nearly every step): such a step is instead seeded with the boxes track_box derives from the device's previous keypoints
    -- the boxes a tracked step would have used -- so that the tracked plan runs at that batch size.  Returns the number of tracked steps."""
    hs = synth.hand_sides(B)
    e.track_reset()
    e.set_profiling(1)
    tracked = 0
    try:
        prev = None
        for t in range(3):
            fr = frames(seed, t, B, H, W)
            fu8 = to_u8(fr) if u8 else None
            if u8:
                fr = G.preprocess_u8(fu8, H, W)
            if t > 0 and reseed_lost and np.any(prev['lost']):
                c, s, _, _ = e.track_box(prev['kp_hw'], H, W)
                e.track_seed(c, s, H, W)
                prev = dict(prev, lost=np.zeros(B, np.int32))
            nd, nt, nu = e.counter('track_detect_steps'), e.counter('track_tracked_steps'), e.counter('crop_u8_launches')
            o = e.track_step_u8(fu8, hs, want_kpmap=True) if u8 else e.track_step(fr, hs, want_kpmap=True)
            seg_free = no_seg_rows(e)
            timing = e.get_timing()
            detect = t == 0 or bool(np.any(prev['lost']))
            assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (nd + detect, nt + (not detect)), t
            if detect:
                assert not seg_free and timing['HandSegNet'] > 0.0
                full = e.infer_full(fr, hs, outputs=('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw'))
            if t == 0:
                assert np.all(o['detected'] == 1)
                for k in ('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw'):
                    assert np.array_equal(o[k], full[k]), k
            else:
                c, s, _, _ = e.track_box(prev['kp_hw'], H, W)
                if detect:
                    assert np.array_equal(o['detected'], prev['lost'])
                    c = np.where(prev['lost'][:, None] == 1, full['center'], c)
                    s = np.where(prev['lost'] == 1, full['scale'].reshape(-1), s)
                else:
                    tracked += 1
                    assert np.all(o['detected'] == 0) and seg_free and timing['HandSegNet'] == 0.0
                    if u8:
                        assert e.counter('crop_u8_launches') > nu
                assert_step_is_composition(e, o, fr, hs, c, s, H, W)
                assert_step_vs_oracle(o, fr, hs, weights, range(B) if oracle_images is None else oracle_images)
            e.set_profiling(1)
            prev = o
    finally:
        e.set_profiling(0)
    return tracked


def run_seed_loss_redetect(e, B, H, W, seed=11):
    """track_seed with image 1's centre far outside the frame: a tracked step that reports image 1 as lost, then a detect step in which
    the lost images take infer_full's box and the others keep the tracked one; detect steps after track_reset, a change of B and a
    change of the frame size; and the schedule of track_redetect = 2.  Returns how many images kept their tracked box."""
    assert B >= 2
    hs = synth.hand_sides(B)
    f0, f1, f2 = (frames(seed, t, B, H, W) for t in range(3))
    full0 = e.infer_full(f0, hs, outputs=('scale', 'center'))
    center = full0['center'].copy()
    scale = full0['scale'].reshape(-1).copy()
    center[1] = (-5000.0, -7000.0)             # far outside the frame
    e.track_seed(center, scale, H, W)
    nd, nt = e.counter('track_detect_steps'), e.counter('track_tracked_steps')
    o1 = e.track_step(f1, hs)
    assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (nd, nt + 1)
    assert np.all(o1['detected'] == 0)
    assert np.array_equal(o1['center'], center) and np.array_equal(o1['scale'].reshape(-1), scale)
    assert o1['lost'][1] == 1 and np.array_equal(o1['lost'], box_rule_batch(o1['kp_hw'], H, W, 1.25)[2])
    o2 = e.track_step(f2, hs)
    assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (nd + 1, nt + 1)
    assert np.array_equal(o2['detected'], o1['lost'])
    full2 = e.infer_full(f2, hs, outputs=('scale', 'center'))
    tc, ts, _, _ = e.track_box(o1['kp_hw'], H, W)
    exp_c = np.where(o1['lost'][:, None] == 1, full2['center'], tc)
    exp_s = np.where(o1['lost'] == 1, full2['scale'].reshape(-1), ts)
    assert_step_is_composition(e, o2, f2, hs, exp_c, exp_s, H, W)
    kept = int((o1['lost'] == 0).sum())
    # reset, a change of B, a change of the frame size: detect steps
    for what in ('reset', 'B', 'size'):
        if what == 'reset':
            e.track_reset()
            fr, h = f0, hs
        elif what == 'B':
            fr, h = f0[:B - 1], hs[:B - 1]
        else:
            fr, h = frames(seed, 3, B - 1, H - 16, W), hs[:B - 1]
        nd = e.counter('track_detect_steps')
        o = e.track_step(fr, h)
        assert e.counter('track_detect_steps') == nd + 1 and np.all(o['detected'] == 1), what
    # track_redetect = 2: every second step detects and re-boxes EVERY image (detected all 1); a step behind a lost image detects as
    # well and re-boxes the lost ones.  The expected kind of each step follows from (first step, previous lost, steps since a detect).
    e.set_option('track_redetect', '2')
    try:
        e.track_reset()
        prev, since = None, 0
        for t in range(4):
            fresh = t == 0
            sched = since + 1 >= 2
            lost_before = (not fresh) and bool(np.any(prev['lost']))
            detect = fresh or sched or lost_before
            nd, nt = e.counter('track_detect_steps'), e.counter('track_tracked_steps')
            o = e.track_step(frames(seed, t, 1, H, W), hs[:1])
            assert (e.counter('track_detect_steps') - nd, e.counter('track_tracked_steps') - nt) == (int(detect), int(not detect)), t
            if fresh or sched:
                assert np.all(o['detected'] == 1), t
            elif detect:
                assert np.array_equal(o['detected'], prev['lost']), t
            else:
                assert np.all(o['detected'] == 0), t
            since = 0 if detect else since + 1
            prev = o
        # ... and one scheduled step that nothing else can explain: seeded at the frame's centre with scale 10 every keypoint of the
        # tracked step lies within 12.8 pixels of the centre, inside the frame, so nothing is lost -- the step behind it detects only
        # because it is the second one, and re-boxes the image although its flag is 0
        e.track_seed(np.array([[H / 2.0, W / 2.0]], F32), np.array([10.0], F32), H, W)
        nd, nt = e.counter('track_detect_steps'), e.counter('track_tracked_steps')
        oa = e.track_step(frames(seed, 0, 1, H, W), hs[:1])
        assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (nd, nt + 1)
        assert oa['lost'][0] == 0 and oa['detected'][0] == 0
        ob = e.track_step(frames(seed, 1, 1, H, W), hs[:1])
        assert (e.counter('track_detect_steps'), e.counter('track_tracked_steps')) == (nd + 1, nt + 1)
        assert ob['detected'][0] == 1
        full = e.infer_full(frames(seed, 1, 1, H, W), hs[:1], outputs=('scale', 'center'))
        assert np.array_equal(ob['center'], full['center']) and np.array_equal(ob['scale'], full['scale'])
    finally:
        e.set_option('track_redetect', '0')
        e.track_reset()
    return kept
