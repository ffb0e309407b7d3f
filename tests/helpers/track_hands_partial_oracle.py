"""Option "track_hands_partial_detect"  restated in NumPy on top of track_hands_oracle (extended by import), and the
checks the CPU (interpreter) and GPU tests share.

The rule: a detect step of the multi-hand tracker that flags alone caused runs, per chunk, the claimed detection on L = the chunk's
frames that have a valid slot flagged lost or no valid slot, at batch m = |L|, on the device's own HandSegNet score map of a batch made of
those frames; every slot of a frame outside L keeps its box and its valid flag with detected = area = claimed = 0.

The pattern of every case is deterministic, as in track_partial_oracle: track_hands_seed gives a slot meant to be lost a centre far
outside the frame -- its keypoint 12 lands outside, lost = 1 -- and every other valid slot the frame's centre with seed_scale(H, W),
whose crop lies wholly inside the frame, so it cannot be lost.  Every case first asserts that valid / lost pattern."""
import numpy as np

import detect_scale_oracle as DS
import hands_oracle as HO
import track_hands_oracle as TH
import track_oracle as TO
import track_partial_oracle as TP
from hand3d_amd.utils import nv12 as NV
from oracle import general as G

F32 = np.float32
OPTION = 'track_hands_partial_detect'
OUT_KEYS = ('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw', 'confidence', 'lost', 'detected', 'valid', 'area', 'claimed')
COUNTERS = ('track_hands_partial_frames_run', 'track_hands_partial_frames_skipped', 'frame_gather_launches', 'track_hands_detect_steps',
            'track_hands_tracked_steps', 'detect_scale_steps', 'track_partial_frames_run', 'track_partial_frames_skipped')
NEW_ROWS = ('track_hands_partial_index', 'track_hands_slot_gather', 'track_hands_select_pos')
GATHER_ROWS = ('frame_gather', 'preprocess_u8_idx', 'preprocess_nv12_idx', 'downscale_idx', 'downscale_u8_idx', 'downscale_nv12_idx')
SELECT_KEYS = ('center', 'scale', 'valid', 'detected', 'area', 'claimed')

# (B, K, H, W, lost slots, absent slots, frame type, f): the issue's cases; absent slots lie in frames outside L
STEP_CASES = [(4, 2, 64, 64, [(0, 1)], [(2, 1)], 'f32', 1),
              (4, 2, 64, 64, [(3, 0)], [(1, 1)], 'u8', 1),
              (5, 4, 37, 53, [(1, 0), (3, 2)], [(0, 3), (4, 1), (4, 2)], 'f32', 1),
              (4, 2, 70, 100, [(0, 0), (1, 1), (2, 0)], [(3, 1)], 'u8', 3),
              (3, 2, 64, 64, [(1, 0)], [(2, 0)], 'nv12', 2),
              (8, 2, 320, 320, [(5, 1)], [(6, 0)], 'f32', 1)]


# ---- the index lists --------------------------------------------------------------------------------------------------------------
def frame_flags(valid, lost):
    """valid / lost [nb,K] -> bool [nb]: a valid slot is lost, or no slot is valid."""
    v, l = np.asarray(valid) != 0, np.asarray(lost) != 0
    return (v & l).any(axis=1) | ~v.any(axis=1)


def index_rule(valid, lost):
    """-> (idx [m] ascending, pos [nb]: the index in idx or -1, m)."""
    flags = frame_flags(valid, lost)
    idx = np.flatnonzero(flags).astype(np.int32)
    pos = np.full(flags.size, -1, np.int32)
    pos[idx] = np.arange(idx.size, dtype=np.int32)
    return idx, pos, int(idx.size)


INDEX_SHAPES = [(1, 1), (5, 2), (255, 3), (256, 4), (257, 1), (600, 4)]


def flag_patterns(nb, K, rng):
    """name -> (valid, lost) [nb,K] int32.  `lost` also carries set flags on absent slots: those must not count."""
    ones, zeros = np.ones((nb, K), np.int32), np.zeros((nb, K), np.int32)
    P = {'none_lost': (ones, zeros), 'all_lost': (ones, ones)}
    first, last = zeros.copy(), zeros.copy()
    first[0, 0] = 1
    last[nb - 1, K - 1] = 1
    P['first_only'], P['last_only'] = (ones, first), (ones, last)
    b = nb // 2
    one = zeros.copy()
    one[b, K - 1] = 1
    P['one_lost_beside_a_kept_slot'] = (ones, one)          # (K = 1: the frame's only slot)
    v = ones.copy()
    v[b, :] = 0
    v[b, 0] = 1
    l = zeros.copy()
    l[b, 0] = 1
    P['only_valid_slot_lost'] = (v, l)
    v = ones.copy()
    v[b, :] = 0
    P['no_valid_slot'] = (v, zeros)
    l = zeros.copy()
    l[b, :] = 1
    P['lost_flags_on_absent_slots_only'] = (v, l)            # (still flagged: no valid slot)
    v = ones.copy()
    v[b, K - 1] = 0
    l = zeros.copy()
    l[b, K - 1] = 1
    P['lost_flag_on_an_absent_slot'] = (v, l)                # (K > 1: not flagged; K = 1: flagged, no valid slot)
    P['random'] = ((rng.random((nb, K)) < 0.7).astype(np.int32), (rng.random((nb, K)) < 0.2).astype(np.int32))
    P['random_sparse'] = ((rng.random((nb, K)) < 0.95).astype(np.int32), (rng.random((nb, K)) < 0.01).astype(np.int32))
    return P


def assert_index_exact(e, nb, K):
    rng = np.random.default_rng(1000 * nb + K)
    for name, (valid, lost) in flag_patterns(nb, K, rng).items():
        idx, pos, m = e.track_hands_partial_index(valid, lost)
        ridx, rpos, rm = index_rule(valid, lost)
        assert m == rm, (name, nb, K, m, rm)
        assert idx.dtype == np.int32 and pos.dtype == np.int32
        assert np.array_equal(idx, ridx) and np.array_equal(pos, rpos), (name, nb, K)
        assert np.all(np.diff(idx) > 0) and np.array_equal(pos[idx], np.arange(m))
    assert index_rule(*flag_patterns(nb, K, rng)['all_lost'])[2] == nb


# ---- the positional select --------------------------------------------------------------------------------------------------------
def select_rule(pos, keep, det, box_center, box_scale, valid):
    """track_hands_select on the frames with pos >= 0 (their dense results at pos[b]); the others keep box and valid, zeros else."""
    pos, keep = np.asarray(pos), np.asarray(keep) != 0
    o = {'center': np.array(box_center, F32), 'scale': np.array(box_scale, F32), 'valid': np.array(valid, np.int32),
         'detected': np.zeros(keep.shape, np.int32), 'area': np.zeros(keep.shape, np.int32), 'claimed': np.zeros(keep.shape, np.int32)}
    for b in np.flatnonzero(pos >= 0):
        p, k = pos[b], keep[b]
        v = (np.asarray(det['valid'][p]) != 0).astype(np.int32)
        o['center'][b] = np.where(k[:, None], o['center'][b], det['center'][p])
        o['scale'][b] = np.where(k, o['scale'][b], det['scale'][p])
        o['valid'][b] = np.where(k, 1, v)
        o['detected'][b] = np.where(k, 0, v)
        o['area'][b] = np.where(k, 0, v * det['area'][p])
        o['claimed'][b] = det['claimed'][p]
    return o


def assert_select_exact(e, nb, K, seed=0):
    """Random flags and dense results -- NaN boxes (the fall-back of empty_reduce = inf on an empty row / column), det_valid values
    other than 0 / 1 and areas on invalid entries included -- and the two ends m = 0 and m = nb."""
    rng = np.random.default_rng(seed + 100 * nb + K)
    for frac in (0.4, 0.0, 1.0):
        flags = rng.random(nb) < frac if 0.0 < frac < 1.0 else np.full(nb, frac == 1.0)
        idx = np.flatnonzero(flags)
        m = idx.size
        pos = np.full(nb, -1, np.int32)
        pos[idx] = np.arange(m)
        keep = (rng.random((nb, K)) < 0.5).astype(np.int32)
        det = {'center': rng.uniform(-50, 400, (m, K, 2)).astype(F32), 'scale': rng.uniform(0.25, 5.0, (m, K)).astype(F32),
               'valid': rng.integers(0, 3, (m, K)).astype(np.int32), 'area': rng.integers(1, 5000, (m, K)).astype(np.int32),
               'claimed': rng.integers(0, 4, (m, K)).astype(np.int32)}
        if m:
            det['center'][0, 0] = (np.nan, 12.0)
            det['center'][m - 1, K - 1] = (np.inf, np.nan)
            keep[idx[0], 0] = 0          # (the NaN box is taken)
        bc = rng.uniform(0, 300, (nb, K, 2)).astype(F32)
        bs = rng.uniform(1.0, 10.0, (nb, K)).astype(F32)
        valid = (rng.random((nb, K)) < 0.6).astype(np.int32)
        got = e.track_hands_select_pos(pos, keep, det, bc, bs, valid)
        ref = select_rule(pos, keep, det, bc, bs, valid)
        for k in SELECT_KEYS:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=(k == 'center')), (k, nb, K, frac)
        if m:
            assert np.isnan(got['center'][idx[0], 0]).any()          # (at m = K = 1 both NaN boxes are this entry)
        out = ~flags
        assert np.array_equal(got['center'][out], bc[out]) and np.array_equal(got['scale'][out], bs[out]) and np.array_equal(got['valid'][out], valid[out])
        assert not got['detected'][out].any() and not got['area'][out].any() and not got['claimed'][out].any()


def assert_option_values(e):
    try:
        for v in ('0', '1'):
            e.set_option(OPTION, v)
        for v in ('2', 'on'):
            with np.testing.assert_raises_regex(AssertionError, "track_hands_partial_detect wants 0 or 1, got " + v):
                e.set_option(OPTION, v)
    finally:
        e.set_option(OPTION, '0')


# ---- the state machine ------------------------------------------------------------------------------------------------------------
class PartialMachine(TH.Machine):
    """track_hands_oracle.Machine with the partial rule, at detect_scale f (rules 3 and 4 of detect_scale_oracle around the detection):
    boxes_chunked() gives the step's boxes chunk by chunk, fed with the device's own score map of each chunk's detecting frames."""

    def __init__(self, f=1, partial=True, **kw):
        self.f, self.partial = f, partial
        TH.Machine.__init__(self, **kw)

    def plan(self, B, K, H, W, chunks):
        """-> (detect, whole, [L per chunk]): whole = a fresh or scheduled step, or the option off (every chunk detects on all frames)."""
        detect, _ = self.kind(B, K, H, W)
        fresh = self.shape != (B, K, H, W)
        sched = self.redetect > 0 and self.since + 1 >= self.redetect
        whole = detect and (fresh or sched or not self.partial)
        if not detect:
            return False, False, [[] for _ in chunks]
        flags = np.ones(B, bool) if whole else frame_flags(self.valid, self.lost)
        return True, whole, [[b for b in ch if flags[b]] for ch in chunks]

    def boxes_chunked(self, B, K, H, W, chunks, scoremap_of):
        """scoremap_of(L) -> the device's HandSegNet score map of a batch made of the (detection) frames L."""
        detect, whole, Ls = self.plan(B, K, H, W, chunks)
        z = np.zeros((B, K), np.int32)
        if not detect:
            return TH.Machine.boxes(self, B, K, H, W)
        _, keep = self.kind(B, K, H, W)
        if self.shape != (B, K, H, W):
            self.center, self.scale, self.valid = np.zeros((B, K, 2), F32), np.ones((B, K), F32), z.copy()
        o = {'detect': True, 'center': self.center.copy(), 'scale': self.scale.copy(), 'valid': self.valid.copy(), 'detected': z.copy(),
             'area': z.copy(), 'claimed': z.copy()}
        for L in Ls:
            if not L:
                continue
            sm = scoremap_of(L)
            if self.f > 1:
                r = DS.masks_keep_rule_at(sm, K, keep[L], self.center[L], self.scale[L], self.f, self.min_area)
            else:
                r = TH.masks_keep_rule(sm, K, keep[L], self.center[L], self.scale[L], self.min_area)
            k = keep[L] != 0
            o['center'][L] = np.where(k[..., None], self.center[L], r['center'])
            o['scale'][L] = np.where(k, self.scale[L], r['scale'])
            o['valid'][L] = np.where(k, 1, r['valid'])
            o['detected'][L] = np.where(k, 0, r['valid'])
            o['area'][L] = np.where(k, 0, r['valid'] * r['area'])
            o['claimed'][L] = r['claimed']
        return o


# ---- scenarios ----------------------------------------------------------------------------------------------------------------------
def seed_slots(B, K, H, W, lost, absent):
    """-> (center [B,K,2], scale [B,K], valid [B,K]) for track_hands_seed."""
    center = np.tile(np.array([H / 2.0, W / 2.0], F32), (B, K, 1))
    scale = np.full((B, K), TP.seed_scale(H, W), F32)
    valid = np.ones((B, K), np.int32)
    for b, j in lost:
        center[b, j] = TP.FAR
        scale[b, j] = 1.0
    for b, j in absent:
        valid[b, j] = 0
    return center, scale, valid


def lost_pattern(B, K, lost):
    p = np.zeros((B, K), np.int32)
    for b, j in lost:
        p[b, j] = 1
    return p


class Frames(object):
    """The frames of step t in the form `kind` ('f32' | 'u8' | 'nv12'): what the step is given, the float32 frame its crop sees, and the
    detection frame of a list of frames by the engine's own per-ops."""

    def __init__(self, e, seed, t, B, H, W, kind, f):
        self.e, self.kind, self.f, self.H, self.W = e, kind, f, H, W
        fr = TO.frames(seed, t, B, H, W)
        self.u8 = None
        if kind == 'f32':
            self.f32 = fr
        else:
            self.u8 = TO.to_u8(fr)
            if kind == 'nv12':
                self.y, self.uv = NV.rgb_to_nv12(self.u8)
                self.u8 = e.nv12_to_rgb(self.y, self.uv)          # (what every NV12 call is defined on)
            self.f32 = G.preprocess_u8(self.u8, H, W)

    def step(self, hs, K, want_kpmap=True):
        e = self.e
        if self.kind == 'f32':
            return e.track_hands_step(self.f32, hs, K, want_kpmap=want_kpmap)
        if self.kind == 'u8':
            return e.track_hands_step_u8(self.u8, hs, K, want_kpmap=want_kpmap)
        return e.track_hands_step_nv12(self.y, self.uv, hs, K, want_kpmap=want_kpmap)

    def detection_frames(self, L):
        """The batch HandSegNet sees for the frames L: hp3d_downscale* at f > 1, the (normalised) frames themselves at f = 1."""
        L = np.asarray(L, np.int64)
        if self.f == 1:
            return self.f32[L]
        return self.e.downscale(self.f32[L], self.f) if self.kind == 'f32' else self.e.downscale_u8(self.u8[L], self.f)

    def gather_row(self):
        if self.f == 1:
            return {'f32': 'frame_gather', 'u8': 'preprocess_u8_idx', 'nv12': 'preprocess_nv12_idx'}[self.kind]
        return {'f32': 'downscale_idx', 'u8': 'downscale_u8_idx', 'nv12': 'downscale_nv12_idx'}[self.kind]


def chunks_of(B, K, micro_batch=None):
    import hands_compact_oracle as HC
    per = HC.chunk_frames(B, K, micro_batch) if micro_batch else HC.chunk_frames(B, K)
    return [list(range(b0, min(b0 + per, B))) for b0 in range(0, B, per)]


def run_two_steps(e, option, B, K, H, W, lost, absent, kind='f32', f=1, seed=21, micro_batch=None, compact='0', redetect='0'):
    """Seed, a tracked step that loses exactly `lost`, then the next step under profiling.  Returns a dict: o1, o2, rows, counter deltas
    of the second step, the Frames of both steps, the machine state before the second step (a PartialMachine advanced over step 1)."""
    hs = HO.hand_sides(B, K)
    e.set_option(OPTION, option)
    e.set_option('detect_scale', str(f))
    e.set_option('hands_compact', compact)
    e.set_option('track_redetect', redetect)
    if micro_batch is not None:
        e.set_option('micro_batch', str(micro_batch))
    try:
        c, s, v = seed_slots(B, K, H, W, lost, absent)
        e.track_hands_seed(c, s, v, H, W)
        m = PartialMachine(f=f, partial=option == '1', redetect=int(redetect))
        m.seed(c, s, v, H, W)
        f0 = Frames(e, seed, 0, B, H, W, kind, f)
        o1 = f0.step(hs, K)
        # the intended pattern, first of all
        assert np.array_equal(o1['valid'], v), o1['valid']
        assert np.array_equal(o1['lost'], lost_pattern(B, K, lost)), o1['lost']
        assert not o1['detected'].any() and not o1['area'].any() and not o1['claimed'].any()
        step1 = m.boxes(B, K, H, W)
        assert not step1['detect']
        m.advance(step1, o1['kp_hw'], B, K, H, W)
        f1 = Frames(e, seed, 1, B, H, W, kind, f)
        n0 = {k: e.counter(k) for k in COUNTERS}
        e.set_profiling(1)
        try:
            o2 = f1.step(hs, K)
            rows = [r[0] for r in e.profile()]
        finally:
            e.set_profiling(0)
        dn = {k: e.counter(k) - n0[k] for k in COUNTERS}
    finally:
        e.set_option(OPTION, '0')
        e.set_option('detect_scale', '1')
        e.set_option('hands_compact', '0')
        e.set_option('track_redetect', '0')
        if micro_batch is not None:
            e.set_option('micro_batch', 'auto')
        e.track_hands_reset()
    return {'o1': o1, 'o2': o2, 'rows': rows, 'dn': dn, 'f0': f0, 'f1': f1, 'machine': m, 'hs': hs, 'seed': (c, s, v)}


def chain_boxes(e, src, K, keep, center, scale, f):
    """The per-op chain on the detection frames `src` of L with L's own keep flags and frame boxes: hp3d_handsegnet ->
    (hp3d_boxes_to_detect ->) hp3d_masks_from_scoremap_keep (-> hp3d_boxes_to_frame).  Returns (its dict, the score map)."""
    sm = e.handsegnet(src)
    kc, ks = e.boxes_to_detect(center, scale, f) if f > 1 else (center, scale)
    r = e.masks_from_scoremap(sm, K, keep=(keep, kc, ks))
    if f > 1:
        r['center'], r['crop_size'], r['scale'] = e.boxes_to_frame(r['center'], r['crop_size'], f)
    return r, sm


def assert_rows_and_counters(res, B, K, f, chunks, Ls, whole_step=False):
    rows, dn, f1 = res['rows'], res['dn'], res['f1']
    partial = [i for i, ch in enumerate(chunks) if 0 < len(Ls[i]) < len(ch)]
    whole = [i for i, ch in enumerate(chunks) if len(Ls[i]) == len(ch)]
    run = sum(len(Ls[i]) for i in partial)
    skipped = sum(len(chunks[i]) - len(Ls[i]) for i in partial)
    print('partial chunks %s whole %s: frames run %d skipped %d; counters %s' % (partial, whole, run, skipped, dn))
    assert not whole_step or not partial
    assert (dn['track_hands_partial_frames_run'], dn['track_hands_partial_frames_skipped']) == (run, skipped)
    assert (dn['track_partial_frames_run'], dn['track_partial_frames_skipped']) == (0, 0)          # the single-hand tracker's: untouched
    assert (dn['track_hands_detect_steps'], dn['track_hands_tracked_steps'], dn['detect_scale_steps']) == (1, 0, int(f > 1))
    n_det = len(partial) + len(whole)
    assert rows.count('seg_upsample_softmax') == n_det and rows.count('mask_grow_multi') == n_det
    for r in NEW_ROWS:
        assert rows.count(r) == len(partial), (r, rows)
    assert rows.count('track_hands_select') == len(whole)
    assert rows.count('track_hands_box') == len(chunks)
    for r in GATHER_ROWS:
        assert rows.count(r) == (len(partial) if r == f1.gather_row() else 0), (r, rows)
    assert dn['frame_gather_launches'] == rows.count('frame_gather')
    if f > 1:
        assert rows.count('box_to_detect') == n_det and rows.count('box_to_frame') == n_det
    return partial, whole


def assert_partial_step(e_on, e_off, B, K, H, W, lost, absent, kind='f32', f=1, micro_batch=None, seed=21, compare_off=True):
    """The two steps on e_on with the option on (and on e_off with it off): rows and counters per chunk, the boxes of L against the
    per-op chain on the gathered frames, every STEP_KEYS output against the extended machine, the composition of the back half, and slot
    by slot against the option-off run: bit-equal for every kept slot outside L; absent slots outside L stay absent."""
    res = run_two_steps(e_on, '1', B, K, H, W, lost, absent, kind, f, seed, micro_batch)
    o1, o2, f1, m, hs = res['o1'], res['o2'], res['f1'], res['machine'], res['hs']
    chunks = chunks_of(B, K, micro_batch)
    detect, whole_step, Ls = m.plan(B, K, H, W, chunks)
    assert detect and not whole_step
    expect_L = sorted(set(b for b, _ in lost))          # (no frame of these cases is without a valid slot)
    assert sorted(b for L in Ls for b in L) == expect_L
    assert_rows_and_counters(res, B, K, f, chunks, Ls)
    # the boxes of L: the per-op chain on the gathered frames, bit for bit
    _, keep = m.kind(B, K, H, W)
    maps = {}
    for L in Ls:
        if not L:
            continue
        r, sm = chain_boxes(e_on, f1.detection_frames(L), K, keep[L], m.center[L], m.scale[L], f)
        maps[tuple(L)] = sm
        free = keep[L] == 0
        assert np.array_equal(o2['center'][L][free], r['center'][free], equal_nan=True) and np.array_equal(o2['scale'][L][free], r['scale'][free])
        assert np.array_equal(o2['valid'][L][free], r['valid'][free]) and np.array_equal(o2['detected'][L][free], r['valid'][free])
        assert np.array_equal(o2['area'][L][free], (r['valid'] * r['area'])[free]) and np.array_equal(o2['claimed'][L], r['claimed'])
        kept = ~free
        assert np.array_equal(o2['center'][L][kept], m.center[L][kept]) and np.array_equal(o2['scale'][L][kept], m.scale[L][kept])
        assert np.all(o2['valid'][L][kept] == 1) and not o2['detected'][L][kept].any() and not o2['area'][L][kept].any()
    # every STEP_KEYS output against the extended machine, fed with the same score maps
    exp = m.boxes_chunked(B, K, H, W, chunks, lambda L: maps[tuple(L)])
    for k in TH.STEP_KEYS:
        assert np.array_equal(o2[k], exp[k], equal_nan=(k == 'center')), (k, o2[k].tolist() if o2[k].size < 64 else None, exp[k].tolist() if exp[k].size < 64 else None)
    outside = np.array([b for b in range(B) if b not in expect_L], np.int64)
    assert not o2['detected'][outside].any() and not o2['area'][outside].any() and not o2['claimed'][outside].any()
    # the composition of the back half, chunk by chunk (the same kernels at the same shapes)
    for ch in chunks:
        TH.compose_slots(e_on, f1.f32[ch], hs[ch], {k: None if v is None else v[ch] for k, v in o2.items()}, H, W)
    lost2 = m.advance(exp, o2['kp_hw'], B, K, H, W)
    assert np.array_equal(o2['lost'], lost2)
    # absent slots outside L stay absent on the fall-back box
    v1 = res['seed'][2]
    for b in outside:
        for j in np.flatnonzero(v1[b] == 0):
            assert o2['valid'][b, j] == 0 and np.all(o2['center'][b, j] == TH.fallback_center()) and o2['scale'][b, j] == TH.FALLBACK_SCALE
            assert o2['detected'][b, j] == 0 and o2['area'][b, j] == 0 and o2['claimed'][b, j] == 0
    if not compare_off:
        return res
    off = run_two_steps(e_off, '0', B, K, H, W, lost, absent, kind, f, seed, micro_batch)
    p1, p2 = off['o1'], off['o2']
    assert off['dn']['track_hands_partial_frames_run'] == 0 and off['dn']['track_hands_partial_frames_skipped'] == 0 and off['dn']['frame_gather_launches'] == 0
    assert not [r for r in off['rows'] if r in NEW_ROWS + GATHER_ROWS]
    for k in OUT_KEYS:
        assert np.array_equal(o1[k], p1[k]), k          # the tracked step: the option changes nothing
    kept_out = np.zeros((B, K), bool)
    kept_out[outside] = v1[outside] != 0
    assert kept_out.any()
    print('claimed of the kept slots outside L: on %s off %s' % (o2['claimed'][kept_out].tolist(), p2['claimed'][kept_out].tolist()))
    for k in OUT_KEYS:
        if k == 'claimed':
            # The rule gives a slot of a frame outside L claimed = 0: nothing was looked for in that frame.  The whole-batch step counts
            # there the objects the kept slot claims (measured on the first case: on [0, 0, 0, 0, 0], off [1, 0, 1, 2, 0]), and no step
            # that skips HandSegNet on the frame can know that count -- so `claimed` is held to the rule, not to the option-off run.
            assert not o2[k][kept_out].any()
            continue
        assert np.array_equal(o2[k][kept_out], p2[k][kept_out]), k          # EVERY other output of a kept slot outside L
    for b in expect_L:          # printed, not asserted: HandSegNet's kernel plan follows m; the per-op chain above is the authority
        print('frame %d of L vs option off: |center| %.3e |scale| %.3e |kpmap| %.3e |coord3d| %.3e valid %s / %s' % (
            b, float(np.nanmax(np.abs(o2['center'][b] - p2['center'][b]))), float(np.abs(o2['scale'][b] - p2['scale'][b]).max()),
            float(np.abs(o2['kpmap'][b] - p2['kpmap'][b]).max()), float(np.abs(o2['coord3d'][b] - p2['coord3d'][b]).max()),
            o2['valid'][b].tolist(), p2['valid'][b].tolist()))
    return res


def assert_chunks(e_on, e_off, H=64, W=64):
    """B = 5, K = 2, two frames per chunk, lost slots in frames 1 and 4: a partial chunk, a chunk enqueued as a tracked one and a whole
    chunk in ONE detect step; detected is nonzero in frames 1 and 4 only."""
    B, K = 5, 2
    assert chunks_of(B, K, 4) == [[0, 1], [2, 3], [4]]
    res = assert_partial_step(e_on, e_off, B, K, H, W, [(1, 0), (4, 1)], [(2, 1)], 'f32', 1, micro_batch=4)
    rows = res['rows']
    assert rows.count('track_hands_select_pos') == 1 and rows.count('track_hands_select') == 1 and rows.count('seg_upsample_softmax') == 2
    d = res['o2']['detected']
    assert not d[[0, 2, 3]].any()
    return res


def assert_fresh_and_scheduled_whole(e_on, e_off, H=64, W=64):
    """With the option on a scheduled step (track_redetect = 2, one slot lost as well) and a fresh step run whole: track_hands_select
    rows, no _pos row, no gather, the new counters do not move, and every output equals the option-off engine bit for bit."""
    B, K = 3, 2
    args = (B, K, H, W, [(1, 0)], [(2, 1)])
    on = run_two_steps(e_on, '1', *args, redetect='2')
    off = run_two_steps(e_off, '0', *args, redetect='2')
    chunks = chunks_of(B, K)
    assert_rows_and_counters(on, B, K, 1, chunks, [list(ch) for ch in chunks], whole_step=True)
    assert not [r for r in on['rows'] if r in NEW_ROWS + GATHER_ROWS] and on['rows'] == off['rows']
    for k in OUT_KEYS:
        assert np.array_equal(on['o1'][k], off['o1'][k]) and np.array_equal(on['o2'][k], off['o2'][k], equal_nan=True), k
    hs = HO.hand_sides(B, K)
    fr = TO.frames(33, 0, B, H, W)
    out = {}
    for e, opt in ((e_on, '1'), (e_off, '0')):
        e.set_option(OPTION, opt)
        try:
            e.track_hands_reset()
            n0 = e.counter('track_hands_partial_frames_run'), e.counter('track_hands_partial_frames_skipped')
            e.set_profiling(1)
            try:
                o = e.track_hands_step(fr, hs, K, want_kpmap=True)
                rows = [r[0] for r in e.profile()]
            finally:
                e.set_profiling(0)
            assert 'track_hands_select' in rows and not [r for r in rows if r in NEW_ROWS + GATHER_ROWS]
            assert (e.counter('track_hands_partial_frames_run'), e.counter('track_hands_partial_frames_skipped')) == n0
            out[opt] = o
        finally:
            e.set_option(OPTION, '0')
            e.track_hands_reset()
    for k in OUT_KEYS:
        assert np.array_equal(out['1'][k], out['0'][k], equal_nan=True), k


def assert_compact_composes(e_on, H=64, W=64):
    """hands_compact = 1 with the option, (4, 2, H, W), slot (0, 1) lost, slot (2, 1) absent outside L: boxes and flags are those of the
    uncompacted partial step; behind the boxes the compacted outputs are what hands_compact_oracle checks for a compacted detect step:
    the composition at batch m = the valid slots, zeros for absent slots, one wait for the detecting chunk."""
    import hands_compact_oracle as HC
    B, K, lost, absent = 4, 2, [(0, 1)], [(2, 1)]
    plain = run_two_steps(e_on, '1', B, K, H, W, lost, absent)
    c0 = HC.counters(e_on)
    res = run_two_steps(e_on, '1', B, K, H, W, lost, absent, compact='1')
    c1 = HC.counters(e_on)
    o2, rows = res['o2'], res['rows']
    for k in TH.STEP_KEYS:
        assert np.array_equal(o2[k], plain['o2'][k], equal_nan=True), k
    for r in NEW_ROWS:
        assert rows.count(r) == 1, r
    assert rows.index('track_hands_select_pos') < rows.index('slot_gather') < rows.index('crop_and_resize_idx')
    assert 'slot_scatter' in rows and 'track_hands_select' not in rows and 'crop_and_resize' not in rows
    back, ms = HC.expected_back_half(e_on, res['f1'].f32, res['hs'], o2['center'], o2['scale'], o2['valid'], K, B)
    HC.assert_back_half(o2, back)
    HC.assert_absent_rule(o2, o2['valid'])
    assert o2['valid'][2, 1] == 0 and ms == [int(o2['valid'].sum())] and ms[0] < B * K
    # both steps were compacted (the tracked one has its flags on the host: no wait; the detect one waits once)
    m1 = int(res['o1']['valid'].sum())
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (m1 + ms[0], 2 * B * K - m1 - ms[0], 1)
    v = o2['valid'] != 0
    for k in ('crop', 'center', 'scale'):          # (bit-equal where the kernel plan does not follow m)
        assert np.array_equal(o2[k][v], plain['o2'][k][v], equal_nan=True), k
    return res


def assert_dev_form_equals_host_form(e, H=64, W=64):
    B, K, lost, absent = 3, 2, [(1, 0)], [(2, 1)]
    host = run_two_steps(e, '1', B, K, H, W, lost, absent)
    assert host['dn']['track_hands_partial_frames_run'] == 1
    hs = host['hs']
    shapes = {k: (v.shape, v.dtype) for k, v in e._track_hands_outputs(B, K, True).items()}
    bufs = {k: e.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    ins = [e.to_device(hs), e.to_device(host['f0'].f32), e.to_device(host['f1'].f32)]
    e.set_option(OPTION, '1')
    try:
        e.track_hands_seed(*host['seed'], H, W)
        args = {k: int(v) for k, v in bufs.items()}
        e.track_hands_step_dev(B, H, W, K, ins[1], ins[0], **args)
        e.sync()
        assert np.array_equal(e.to_host(bufs['lost'], (B, K), np.int32), lost_pattern(B, K, lost))
        n = e.counter('track_hands_partial_frames_run'), e.counter('frame_gather_launches')
        e.track_hands_step_dev(B, H, W, K, ins[2], ins[0], **args)
        e.sync()
        assert (e.counter('track_hands_partial_frames_run'), e.counter('frame_gather_launches')) == (n[0] + 1, n[1] + 1)
        for k, (s, dt) in shapes.items():
            assert np.array_equal(e.to_host(bufs[k], s, dt), host['o2'][k], equal_nan=True), k
    finally:
        e.set_option(OPTION, '0')
        e.track_hands_reset()
        for b in list(bufs.values()) + ins:
            b.free()


def assert_nv12_equals_u8(e, H=64, W=64):
    """The NV12 host form equals the uint8 form on the converted frames bit for bit, both steps, partial detection on."""
    B, K, lost, absent = 3, 2, [(1, 1)], [(0, 1)]
    nv = run_two_steps(e, '1', B, K, H, W, lost, absent, kind='nv12')
    assert nv['dn']['track_hands_partial_frames_run'] == 1 and nv['rows'].count('preprocess_nv12_idx') == 1
    hs = nv['hs']
    e.set_option(OPTION, '1')
    try:
        e.track_hands_seed(*nv['seed'], H, W)
        u1 = e.track_hands_step_u8(nv['f0'].u8, hs, K, want_kpmap=True)
        n = e.counter('track_hands_partial_frames_run')
        u2 = e.track_hands_step_u8(nv['f1'].u8, hs, K, want_kpmap=True)
        assert e.counter('track_hands_partial_frames_run') == n + 1
    finally:
        e.set_option(OPTION, '0')
        e.track_hands_reset()
    for k in OUT_KEYS:
        assert np.array_equal(nv['o1'][k], u1[k]) and np.array_equal(nv['o2'][k], u2[k], equal_nan=True), k


def assert_ignored_elsewhere(e, H, W):
    """hp3d_infer_hands, hp3d_track_step and hp3d_infer_full are bit-equal with the option on and off; the counters do not move."""
    from hand3d_amd import synth
    fr, hs, hsk = TO.frames(41, 0, 2, H, W), synth.hand_sides(2), HO.hand_sides(2, 2)
    n0 = e.counter('track_hands_partial_frames_run'), e.counter('track_hands_partial_frames_skipped')
    res = {}
    for opt in ('0', '1'):
        e.set_option(OPTION, opt)
        try:
            full = e.infer_full(fr, hs, outputs=('scoremap', 'crop', 'scale', 'center', 'coord3d', 'kp_hw'))
            hands = e.infer_hands(fr, hsk, 2)
            e.track_seed(*TP.seed_boxes(2, H, W, [1]), H, W)          # a tracked step that loses image 1, then its detect step
            t1 = e.track_step(fr, hs)
            t2 = e.track_step(fr, hs)
            assert t1['lost'].tolist() == [0, 1] and t2['detected'].tolist() == [0, 1]
        finally:
            e.set_option(OPTION, '0')
            e.track_reset()
        res[opt] = (full, hands, t1, t2)
    for a, b in zip(res['0'], res['1']):
        for k, v in a.items():
            if v is not None:
                assert np.array_equal(v, b[k], equal_nan=True), k
    assert (e.counter('track_hands_partial_frames_run'), e.counter('track_hands_partial_frames_skipped')) == n0
