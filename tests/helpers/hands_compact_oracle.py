"""Option "hands_compact"  restated in NumPy on top of track_hands_oracle, hands_oracle and track_oracle, for the CPU
(interpreter) and the GPU tests.

Per chunk of frames, idx = the slots b K + j with valid = 1, ascending.  A valid slot idx[i] returns what the existing ops give at batch m
on frame idx[i] // K, the slot's box and its hand_side (track_oracle.compose on the gathered inputs, no tolerance); an absent slot
returns zeros behind the crop, confidence = lost = 0, and keeps its fall-back box.  A chunk without an absent slot is the uncompacted
call."""
import numpy as np

import track_oracle as TO
import track_hands_oracle as THO
from oracle import general as G

F32 = np.float32
BACK_KEYS = ('crop', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw')
NEW_ROWS = ('slot_gather', 'slot_scatter', 'crop_and_resize_idx', 'crop_and_resize_idx_u8')
COUNTERS = ('hands_compact_slots_run', 'hands_compact_slots_skipped', 'hands_compact_waits')
last_rows = []          # the profile rows of the last step_and_check / infer_hands_and_check


def idx_pos(valid):
    """valid [ns] -> (idx [m] ascending, pos [ns]: the dense index or -1)."""
    v = np.asarray(valid).reshape(-1) != 0
    idx = np.flatnonzero(v).astype(np.int32)
    pos = np.full(v.size, -1, np.int32)
    pos[idx] = np.arange(idx.size, dtype=np.int32)
    return idx, pos


def chunk_frames(B, K, micro_batch=32):
    """Frames per chunk of a multi-hand call (float32 trunks): at most micro_batch / K, at least one."""
    return max(1, min(B, micro_batch, max(1, micro_batch // K)))


def counters(e):
    return tuple(e.counter(k) for k in COUNTERS)


def expected_back_half(e, frame, hs, center, scale, valid, K, per_chunk):
    """The back-half outputs of a compacted call, [B,K,...]: per chunk the composition at batch m on the gathered inputs scattered to
    the slot layout, zeros for absent slots; a chunk without an absent slot is the composition at batch ns.  Also 'confidence' (0 for
    absent slots) and the per-chunk m."""
    B = frame.shape[0]
    out = {'crop': np.zeros((B, K, 256, 256, 3), F32), 'kpmap': np.zeros((B, K, 256, 256, 21), F32), 'coord3d': np.zeros((B, K, 21, 3), F32),
           'kp_crop': np.zeros((B, K, 21, 2), np.int32), 'kp_hw': np.zeros((B, K, 21, 2), np.float64), 'confidence': np.zeros((B, K), F32)}
    ms = []
    for b0 in range(0, B, per_chunk):
        sl = slice(b0, min(B, b0 + per_chunk))
        idx, _ = idx_pos(valid[sl])
        ms.append(int(idx.size))
        if idx.size == 0:
            continue
        fr, h = frame[sl], hs[sl].reshape(-1, 2)
        c, s = center[sl].reshape(-1, 2), scale[sl].reshape(-1)
        comp = TO.compose(e, fr[idx // K], h[idx], c[idx], s[idx])
        for k in BACK_KEYS:
            v = out[k][sl]
            flat = v.reshape((-1,) + v.shape[2:])
            flat[idx] = comp[k]
            out[k][sl] = flat.reshape(v.shape)
        conf = out['confidence'][sl].reshape(-1)
        conf[idx] = TO.confidence(comp['sm'])
        out['confidence'][sl] = conf.reshape(out['confidence'][sl].shape)
    return out, ms


def assert_back_half(o, exp, keys=BACK_KEYS + ('confidence',)):
    for k in keys:
        if o.get(k) is None:
            continue
        assert np.array_equal(o[k], exp[k]), k


def assert_absent_rule(o, valid, tracker=True):
    """Rule 3 on the engine's outputs alone: everything behind the crop is exactly 0 for an absent slot."""
    a = np.asarray(valid) == 0
    for k in BACK_KEYS:
        if o.get(k) is not None:
            assert not o[k][a].any(), k
    if tracker:
        for k in ('confidence', 'lost', 'detected', 'area'):
            assert not o[k][a].any(), k


def step_and_check(e, m, frame, hs, K, per_chunk, u8=None, scoremap=None, want_kpmap=True):
    """track_hands_oracle.step_and_check with the option on: one engine step against the restated machine `m` and the absent rule.
    Returns (outputs, detect, per-chunk m)."""
    B, H, W, _ = frame.shape
    detect, _ = m.kind(B, K, H, W)
    nd, nt = e.counter('track_hands_detect_steps'), e.counter('track_hands_tracked_steps')
    c0 = counters(e)
    e.set_profiling(1)
    try:
        o = e.track_hands_step_u8(u8, hs, K, want_kpmap=want_kpmap) if u8 is not None else e.track_hands_step(frame, hs, K, want_kpmap=want_kpmap)
        rows = [r[0] for r in e.profile()]
        seg_free = THO.no_seg_rows(e)
    finally:
        e.set_profiling(0)
    last_rows[:] = rows
    assert (e.counter('track_hands_detect_steps') - nd, e.counter('track_hands_tracked_steps') - nt) == (int(detect), int(not detect))
    assert seg_free == (not detect) and ('track_hands_select' in rows) == detect and 'track_hands_box' in rows
    if detect and scoremap is None:
        scoremap = e.handsegnet(frame)
    exp = m.boxes(B, K, H, W, scoremap)
    for k in THO.STEP_KEYS:
        assert np.array_equal(o[k], exp[k]), (k, o[k].tolist() if o[k].size < 64 else None, exp[k].tolist() if exp[k].size < 64 else None)
    back, ms = expected_back_half(e, frame, hs, o['center'], o['scale'], o['valid'], K, per_chunk)
    assert_back_half(o, back)
    assert_absent_rule(o, o['valid'])
    v = o['valid'].reshape(-1) != 0
    assert np.array_equal(o['crop'].reshape(B * K, 256, 256, 3)[v],
                          G.crop_image_from_xy(np.repeat(frame, K, axis=0)[v], o['center'].reshape(-1, 2)[v], 256, o['scale'].reshape(-1)[v]))
    lost = m.advance(exp, o['kp_hw'], B, K, H, W)
    assert np.array_equal(o['lost'], lost)
    nchunks = len(ms)
    c1 = counters(e)
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (sum(ms), B * K - sum(ms), nchunks if detect else 0)
    sizes = [min(B, b0 + per_chunk) - b0 for b0 in range(0, B, per_chunk)]
    partial = any(mm < nb * K for mm, nb in zip(ms, sizes))
    assert ('slot_scatter' in rows) == partial
    assert ('slot_gather' in rows) == any(0 < mm < nb * K for mm, nb in zip(ms, sizes))
    for k, val in o.items():
        if val is not None and val.dtype.kind == 'f':
            assert np.all(np.isfinite(val)), k
    return o, detect, ms


def infer_hands_and_check(e, frame, hs, K, per_chunk, off=None, want_mask=True):
    """hp3d_infer_hands with the option on (the caller has set it): everything in front of the crop equals the option-off call `off`
    bit for bit; behind it the composition at batch m and the absent rule.  Returns (outputs, per-chunk m)."""
    B = frame.shape[0]
    c0 = counters(e)
    e.set_profiling(1)
    try:
        o = e.infer_hands(frame, hs, K, want_mask=want_mask)
        rows = [r[0] for r in e.profile()]
    finally:
        e.set_profiling(0)
    last_rows[:] = rows
    if off is not None:
        for k in ('scoremap', 'mask', 'valid', 'area', 'center', 'scale'):
            if off.get(k) is not None:
                assert np.array_equal(o[k], off[k]), k
    back, ms = expected_back_half(e, frame, hs, o['center'], o['scale'], o['valid'], K, per_chunk)
    assert_back_half(o, back, BACK_KEYS)
    assert_absent_rule(o, o['valid'], tracker=False)
    c1 = counters(e)
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (sum(ms), B * K - sum(ms), len(ms))
    if sum(ms) == 0:
        assert not [r for r in rows if r.startswith('PoseNet2D/')]
    return o, ms
