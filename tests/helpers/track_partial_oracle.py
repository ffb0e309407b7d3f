"""Checks the CPU (interpreter) and GPU tests of option "track_partial_detect"  share.

The lost set of every case is deterministic (tests/test_track.py's seeding): track_seed gives the frames meant to be lost a centre far
outside the frame -- their keypoint 12 lands outside, lost = 1 -- and the others the frame's centre with a scale whose crop (256 / scale
pixels) lies wholly inside the frame, so every keypoint of theirs is inside and lost = 0.  Every case first asserts that pattern."""
import numpy as np

import detect_scale_oracle as DS
import track_oracle as TO
from hand3d_amd import synth
from oracle import general as G

F32 = np.float32
OUT_KEYS = ('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw', 'confidence', 'lost', 'detected')
PARTIAL_COUNTERS = ('track_partial_frames_run', 'track_partial_frames_skipped', 'frame_gather_launches', 'track_detect_steps',
                    'track_tracked_steps', 'crop_u8_launches', 'detect_scale_steps')
FAR = (-5000.0, -7000.0)

GATHER_SHAPES = [(5, 37, 53), (4, 32, 32)]          # 23 532 bytes per frame: the 4-byte gather | 12 288: the 16-byte one


def gather_indices(B):
    return [[0], [B - 1], [1, 3], list(range(B))]


def assert_gather_frames_exact(e, B, H, W, f, idx, u8, seed=0):
    """hp3d_gather_frames against the existing per-ops on the gathered frames, bit for bit."""
    rng = np.random.default_rng(seed + H * 1000 + W + 7 * f)
    idx = np.asarray(idx, np.int32)
    if u8:
        x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        ref = e.downscale_u8(x[idx], f) if f > 1 else e.preprocess_u8(x[idx], H, W)
        if f == 1:
            assert np.array_equal(ref, G.preprocess_u8(x[idx], H, W))
    else:
        x = rng.uniform(-0.5, 0.5, (B, H, W, 3)).astype(F32)
        x[:, :2, :3] *= F32(1e4)             # (a sum whose order matters)
        ref = e.downscale(x[idx], f) if f > 1 else x[idx]
    got = e.gather_frames(x, idx, f)
    assert got.dtype == F32 and got.shape == (len(idx),) + DS.detect_shape(H, W, f) + (3,)
    assert np.array_equal(got, ref), (B, H, W, f, idx.tolist(), u8)


def assert_gather_frames_errors(e):
    from hand3d_amd import _lib
    lib, h = e.lib, e.h
    x = np.zeros((3, 16, 16, 3), F32)
    u = np.zeros((3, 16, 16, 3), np.uint8)
    out = np.zeros((3, 16, 16, 3), F32)
    p = _lib._ptr

    def call(img, img8, B, f, idx, m):
        idx = np.asarray(idx, np.int32)
        return lib.hp3d_gather_frames(h, img, img8, B, 16, 16, f, p(idx), m, p(out))
    assert call(p(x), None, 3, 1, [0, 2], 2) == 0
    assert call(None, p(u), 3, 2, [1], 1) == 0
    assert call(p(x), p(u), 3, 1, [0], 1) == -1 and call(None, None, 3, 1, [0], 1) == -1          # both / neither image
    assert call(p(x), None, 3, 1, [0], 0) == -1 and call(p(x), None, 3, 1, [0, 1, 2, 2], 4) == -1       # m outside 1 ... B
    for bad in ([1, 1], [2, 1], [-1, 0], [0, 3]):                                                     # not strictly ascending in [0, B)
        assert call(p(x), None, 3, 1, bad, 2) == -1, bad
    assert call(p(x), None, 3, 0, [0], 1) == -1 and call(p(x), None, 3, 9, [0], 1) == -1              # f outside 1 ... 8
    assert lib.hp3d_gather_frames(h, p(x), None, 3, 16, 16, 1, None, 1, p(out)) == -1
    assert lib.hp3d_gather_frames(None, p(x), None, 3, 16, 16, 1, None, 1, p(out)) == -1


def seed_scale(H, W):
    """A scale whose crop (256 / scale pixels around the frame's centre) lies inside the frame: 25.6 pixels, or 51.2 where they fit."""
    s = 5.0 if min(H, W) >= 52 else 10.0
    assert 256.0 / s <= min(H, W)
    return s


def seed_boxes(B, H, W, lost):
    center = np.tile(np.array([H / 2.0, W / 2.0], F32), (B, 1))
    scale = np.full(B, seed_scale(H, W), F32)
    for b in lost:
        center[b] = FAR
        scale[b] = 1.0
    return center, scale


def pattern(B, lost):
    p = np.zeros(B, np.int32)
    p[list(lost)] = 1
    return p


def case_frames(seed, t, B, H, W, u8):
    """(what the step is given, the float32 frame its crop sees)"""
    fr = TO.frames(seed, t, B, H, W)
    if not u8:
        return fr, fr
    fu8 = TO.to_u8(fr)
    return fu8, G.preprocess_u8(fu8, H, W)


def step(e, given, hs, u8, want_kpmap=True):
    return e.track_step_u8(given, hs, want_kpmap=want_kpmap) if u8 else e.track_step(given, hs, want_kpmap=want_kpmap)


def run_two_steps(e, option, B, H, W, lost, u8, f, seed=21, micro_batch=None):
    """Seed, a tracked step that loses exactly `lost`, then the detect step under profiling.  Returns (o1, o2, rows, counter deltas of
    the detect step, the detect step's float32 frame, what it was given)."""
    hs = synth.hand_sides(B)
    e.set_option('track_partial_detect', option)
    e.set_option('detect_scale', str(f))
    if micro_batch is not None:
        e.set_option('micro_batch', str(micro_batch))
    try:
        c, s = seed_boxes(B, H, W, lost)
        e.track_seed(c, s, H, W)
        g0, _ = case_frames(seed, 0, B, H, W, u8)
        o1 = step(e, g0, hs, u8)
        assert np.array_equal(o1['lost'], pattern(B, lost)), o1['lost']           # the intended pattern, first of all
        assert np.all(o1['detected'] == 0)
        g1, fr1 = case_frames(seed, 1, B, H, W, u8)
        n0 = {k: e.counter(k) for k in PARTIAL_COUNTERS}
        e.set_profiling(1)
        try:
            o2 = step(e, g1, hs, u8)
            rows = [r[0] for r in e.profile()]
        finally:
            e.set_profiling(0)
        dn = {k: e.counter(k) - n0[k] for k in PARTIAL_COUNTERS}
    finally:
        e.set_option('track_partial_detect', '0')
        e.set_option('detect_scale', '1')
        if micro_batch is not None:
            e.set_option('micro_batch', 'auto')
    return o1, o2, rows, dn, fr1, g1


def detected_boxes(e, given, fr, idx, f, u8):
    """The boxes the same ops give on a batch made of the frames idx: hp3d_infer_full's at f = 1, the per-op chain at f > 1."""
    idx = np.asarray(idx, np.int32)
    if f == 1:
        full = e.infer_full(fr[idx], synth.hand_sides(len(idx)), outputs=('scale', 'center'))
        return full['center'], full['scale'].reshape(-1)
    src = e.downscale_u8(given[idx], f) if u8 else e.downscale(given[idx], f)
    assert np.array_equal(e.gather_frames(given, idx, f), src)
    _, c_d, size_d, _, _ = e.mask_from_scoremap(e.handsegnet(src))
    size_d = size_d.reshape(-1)
    center, _, scale = e.boxes_to_frame(c_d, size_d, f)
    rc, _, rs = DS.boxes_to_frame(c_d, size_d, f)
    assert np.array_equal(center, rc, equal_nan=True) and np.array_equal(scale, rs)
    return center, scale.reshape(-1)


def chunks_of(B, mb):
    mb = B if not mb else mb
    return [list(range(b0, min(b0 + mb, B))) for b0 in range(0, B, mb)]


def assert_partial_step(e_on, e_off, B, H, W, lost, u8, f, micro_batch=None, seed=21, compare_off=True):
    """The two steps on e_on with the option on (and on e_off with it off): rows, counters, boxes, the composition, and image by image
    against the option-off run -- bit-equal outside the lost set, to the end-to-end tolerances inside it."""
    lost = sorted(lost)
    hs = synth.hand_sides(B)
    o1, o2, rows, dn, fr1, g1 = run_two_steps(e_on, '1', B, H, W, lost, u8, f, seed, micro_batch)
    pat = pattern(B, lost)
    chunks = chunks_of(B, micro_batch)
    L = [[b for b in ch if pat[b]] for ch in chunks]
    partial = [i for i, ch in enumerate(chunks) if 0 < len(L[i]) < len(ch)]
    whole = [i for i, ch in enumerate(chunks) if len(L[i]) == len(ch)]
    run = sum(len(L[i]) for i in partial)
    skipped = sum(len(chunks[i]) - len(L[i]) for i in partial)
    print('partial chunks %s whole %s: frames run %d skipped %d; counters %s' % (partial, whole, run, skipped, dn))
    # counters: HandSegNet ran at batch m in the partial chunks, the step is ONE detect step
    assert (dn['track_partial_frames_run'], dn['track_partial_frames_skipped']) == (run, skipped)
    assert (dn['track_detect_steps'], dn['track_tracked_steps'], dn['detect_scale_steps']) == (1, 0, int(f > 1))
    # rows: one HandSegNet pass, soft-max and growth per chunk that holds a lost frame, none for the others
    n_det = len(partial) + len(whole)
    assert rows.count('seg_upsample_softmax') == n_det and rows.count('mask_grow') + rows.count('mask_grow_global') == n_det
    assert rows.count('track_partial_index') == len(partial) and rows.count('track_select_pos') == len(partial)
    assert rows.count('track_select') == len(whole) and rows.count('track_box') == len(chunks)
    gather = 'frame_gather' if (f == 1 and not u8) else 'preprocess_u8_idx' if f == 1 else 'downscale_u8_idx' if u8 else 'downscale_idx'
    for r in ('frame_gather', 'preprocess_u8_idx', 'downscale_idx', 'downscale_u8_idx'):
        assert rows.count(r) == (len(partial) if r == gather else 0), (r, rows)
    assert dn['frame_gather_launches'] == rows.count('frame_gather')
    if u8:          # every chunk but a whole one at f = 1 crops straight from the uint8 frame
        assert dn['crop_u8_launches'] == len(chunks) - (len(whole) if f == 1 else 0)
        assert rows.count('preprocess_u8') == (len(whole) if f == 1 else 0)
    # boxes: HandSegNet's on the gathered frames for the lost ones, the tracked ones for the others
    assert np.array_equal(o2['detected'], pat)
    exp_c, exp_s, _, _ = e_on.track_box(o1['kp_hw'], H, W)
    for i in partial + whole:
        c, s = detected_boxes(e_on, g1, fr1, L[i], f, u8)
        exp_c[L[i]] = c
        exp_s[L[i]] = s
    for ch in chunks:          # (the back half ran chunk by chunk: the same kernels at the same shapes)
        TO.assert_step_is_composition(e_on, {k: None if v is None else v[ch] for k, v in o2.items()}, fr1[ch], hs[ch], exp_c[ch], exp_s[ch], H, W)
    if not compare_off:
        return o2
    p1, p2, rows_off, dn_off, _, _ = run_two_steps(e_off, '0', B, H, W, lost, u8, f, seed, micro_batch)
    assert dn_off['track_partial_frames_run'] == 0 and dn_off['track_partial_frames_skipped'] == 0 and dn_off['frame_gather_launches'] == 0
    assert not [r for r in rows_off if r in ('track_partial_index', 'frame_gather', 'preprocess_u8_idx', 'downscale_idx',
                                             'downscale_u8_idx', 'track_select_pos')]
    for k in OUT_KEYS:
        assert np.array_equal(o1[k], p1[k]), k          # the tracked step: the option changes nothing
    keep = np.flatnonzero(pat == 0)
    for k in OUT_KEYS:
        assert np.array_equal(o2[k][keep], p2[k][keep]), k          # EVERY output of an image that kept its box
    for b in lost:          # the lost ones: HandSegNet's kernel plan follows m -- the end-to-end tolerances (track_oracle's)
        dk = float(np.abs(o2['kpmap'][b] - p2['kpmap'][b]).max())
        d3 = float(np.abs(o2['coord3d'][b] - p2['coord3d'][b]).max())
        print('image %d: |center| %.3e |scale| %.3e |kpmap| %.3e |coord3d| %.3e' % (
            b, float(np.abs(o2['center'][b] - p2['center'][b]).max()), float(np.abs(o2['scale'][b] - p2['scale'][b]).max()), dk, d3))
        assert dk < TO.TOL_HEATMAP and d3 < TO.TOL_KP3D, (b, dk, d3)
    return o2


def assert_scheduled_and_fresh_untouched(e, H, W):
    """track_redetect = 2 with the option on, B = 2, image 1 lost: the step behind the tracked one is scheduled as well, re-boxes
    every image and runs as without the option; so does a fresh step."""
    B = 2
    hs = synth.hand_sides(B)
    e.set_option('track_partial_detect', '1')
    e.set_option('track_redetect', '2')
    try:
        c, s = seed_boxes(B, H, W, [1])
        e.track_seed(c, s, H, W)
        n0 = e.counter('track_partial_frames_run'), e.counter('track_partial_frames_skipped')
        o1 = e.track_step(TO.frames(31, 0, B, H, W), hs)
        assert np.array_equal(o1['lost'], [0, 1]) and np.all(o1['detected'] == 0)
        f1 = TO.frames(31, 1, B, H, W)
        e.set_profiling(1)
        try:
            o2 = e.track_step(f1, hs)
            rows = [r[0] for r in e.profile()]
        finally:
            e.set_profiling(0)
        assert np.all(o2['detected'] == 1) and 'track_select' in rows and 'track_select_pos' not in rows and 'frame_gather' not in rows
        full = e.infer_full(f1, hs, outputs=('scale', 'center'))
        assert np.array_equal(o2['center'], full['center']) and np.array_equal(o2['scale'], full['scale'])
        e.track_reset()
        o3 = e.track_step(f1, hs)          # fresh
        assert np.all(o3['detected'] == 1) and np.array_equal(o3['center'], full['center'])
        assert (e.counter('track_partial_frames_run'), e.counter('track_partial_frames_skipped')) == n0
    finally:
        e.set_option('track_partial_detect', '0')
        e.set_option('track_redetect', '0')
        e.track_reset()


def assert_other_entry_points_ignore(e, H, W):
    """hp3d_infer_full and hp3d_track_hands_step with the option on are bit-equal to the option off."""
    import hands_oracle as HO
    fr, hs = TO.frames(41, 0, 1, H, W), synth.hand_sides(1)
    hsk = HO.hand_sides(1, 1)
    res = {}
    n0 = e.counter('track_partial_frames_run')
    for opt in ('0', '1'):
        e.set_option('track_partial_detect', opt)
        try:
            full = e.infer_full(fr, hs, outputs=('scoremap', 'crop', 'scale', 'center', 'coord3d', 'kp_hw'))
            e.track_hands_reset()
            th = e.track_hands_step(fr, hsk, 1)
        finally:
            e.set_option('track_partial_detect', '0')
            e.track_hands_reset()
        res[opt] = (full, th)
    for i in (0, 1):
        for k, v in res['0'][i].items():
            if v is not None:
                assert np.array_equal(v, res['1'][i][k], equal_nan=True), k
    assert e.counter('track_partial_frames_run') == n0
