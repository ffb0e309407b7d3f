"""NumPy restatement of the multi-hand tracker -- the claim rule of a detect step's mask growth and the per-slot state
machine -- and the checks the CPU (interpreter) and GPU tests share.  Built from hands_oracle.hands_rule / masks_rule (the objects and
their order), track_oracle.box_rule / confidence (the per-slot box rule) and oracle.general.

Claim rule, for one image: objects are found as hands_rule finds them (grow inside R from the first arg-max of fg over R, then take the
object out of R; pass cap unchanged).  With o = calc_center_bb's centre of the object, [rmin, rmax] x [cmin, cmax] its bounding box and
(c, s) a kept slot's box, half = 128 / s: the slot claims the object when |o.row - c.row| <= half and |o.col - c.col| <= half, or when
rmin <= c.row <= rmax and cmin <= c.col <= cmax -- float32 op by op, a comparison with a NaN is false.  A claimed object is dropped
(never tested against min_area) and counted for the lowest slot that claims it; the others, if they have min_area pixels, fill the
free slots in the order of discovery, lowest free slot first.  Every growth counts toward the cap of 4 K per image; the loop ends when
an accepted object fills the last free slot, when R is empty, or at the cap (so with no free slot it runs to the end of R or the cap and
`claimed` says which kept slots the map still shows).  No kept slot: hands_rule.  Kept slots and an empty det: every free slot absent.
Kept slots come back as absent slots do."""
import numpy as np

import hands_oracle as HO
import track_oracle as TO
from hand3d_amd import synth
from oracle import general as G

F32 = np.float32
KEEP_KEYS = HO.MASK_KEYS + ('claimed',)


def claim_clauses(obj, c, s):
    """obj [H,W] 0/1 (not empty), box centre c (row, col) and scale s -> (first clause, second clause), float32 op by op."""
    rows, cols = np.nonzero(obj)
    rmin, rmax, cmin, cmax = F32(rows.min()), F32(rows.max()), F32(cols.min()), F32(cols.max())
    o = G.calc_center_bb(obj[None, :, :, None])[0][0]
    c = np.asarray(c, F32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        half = F32(128.0) / F32(s)
        near = bool(np.abs(F32(o[0] - c[0])) <= half) and bool(np.abs(F32(o[1] - c[1])) <= half)
        inside = bool(rmin <= c[0]) and bool(c[0] <= rmax) and bool(cmin <= c[1]) and bool(c[1] <= cmax)
    return near, inside


def claims(obj, c, s):
    return any(claim_clauses(obj, c, s))


def claimed_rule(scoremap, K, keep, kc, ks, min_area=0):
    """One image: scoremap [H,W,2], keep [K], kc [K,2], ks [K] -> (K slot dicts as hands_rule's, claimed int32 [K])."""
    keep = np.asarray(keep).astype(bool)
    claimed = np.zeros(K, np.int32)
    if not keep.any():
        return HO.hands_rule(scoremap, K, min_area), claimed
    fg, det = G.fg_and_detmap(np.asarray(scoremap, F32)[None])
    fg, det = fg[0], det[0]
    H, W = det.shape
    absent = lambda: {'mask': np.zeros((H, W), F32), 'seed': np.array([-1, -1], np.int32), 'valid': 0, 'area': 0}
    slots = [absent() for _ in range(K)]
    free = [j for j in range(K) if not keep[j]]
    R = det.copy()
    k = tries = 0
    while tries < 4 * K and R.any():
        idx = int(np.argmax(np.where(R == 1, fg, -np.inf)))
        seed = np.array([idx // W, idx % W], np.int32)
        obj, _ = G.grow_objectmap(R, seed, early_exit=True)
        R = (R * (1 - obj)).astype(F32)
        tries += 1
        who = [j for j in range(K) if keep[j] and claims(obj, kc[j], ks[j])]
        if who:
            claimed[who[0]] += 1
        elif free and int(obj.sum()) >= min_area:          # (no free slot: dropped, like a claimed one)
            slots[free[k]] = {'mask': obj, 'seed': seed, 'valid': 1, 'area': int(obj.sum())}
            k += 1
            if k == len(free):
                break
    return slots, claimed


def masks_keep_rule(scoremap, K, keep, kc, ks, min_area=0):
    """scoremap [B,H,W,2], keep [B,K], kc [B,K,2], ks [B,K] -> dict like Engine.masks_from_scoremap(keep=...)'s."""
    sm = np.asarray(scoremap, F32)
    B, H, W, _ = sm.shape
    o = {'mask': np.zeros((B, K, H, W), F32), 'center': np.zeros((B, K, 2), F32), 'crop_size': np.zeros((B, K), F32),
         'scale': np.zeros((B, K), F32), 'seed': np.zeros((B, K, 2), np.int32), 'valid': np.zeros((B, K), np.int32),
         'area': np.zeros((B, K), np.int32), 'claimed': np.zeros((B, K), np.int32)}
    for b in range(B):
        slots, o['claimed'][b] = claimed_rule(sm[b], K, keep[b], kc[b], ks[b], min_area)
        for j, s in enumerate(slots):
            center, _, size = G.calc_center_bb(s['mask'][None, :, :, None])
            o['mask'][b, j] = s['mask']
            o['center'][b, j] = center[0]
            o['crop_size'][b, j] = size[0, 0]
            o['scale'][b, j] = G.scale_from_crop_size(size)[0, 0]
            o['seed'][b, j] = s['seed']
            o['valid'][b, j] = s['valid']
            o['area'][b, j] = s['area']
    return o


def as_keep(K, kept):
    """{slot: (row, col, scale)} -> (keep [1,K], center [1,K,2], scale [1,K]); slots not kept carry a box that would claim everything
    if it were looked at (it must not be)."""
    keep, kc, ks = np.zeros((1, K), np.int32), np.zeros((1, K, 2), F32), np.full((1, K), 1e-3, F32)
    for j, (r, c, s) in kept.items():
        keep[0, j], kc[0, j], ks[0, j] = 1, (r, c), s
    return keep, kc, ks


def assert_keep_exact(e, sm, K, keep, min_area=0, both_forms=True):
    """The engine's claimed mask stage equals the rule bit for bit; the LDS and the global form give equal bits (told apart by the
    counters).  Returns the engine's result."""
    ref = masks_keep_rule(sm, K, *keep, min_area=min_area)
    got = e.masks_from_scoremap(sm, K, keep=keep)
    for k in KEEP_KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        assert np.array_equal(got[k], ref[k]), (k, got[k] if got[k].size < 64 else None, ref[k] if ref[k].size < 64 else None)
    if both_forms:
        try:
            e.set_option('mask_grow', 'lds')
            n_m, n_g = e.counter('mask_grow_multi_launches'), e.counter('mask_grow_global_launches')
            lds = e.masks_from_scoremap(sm, K, keep=keep)
            assert (e.counter('mask_grow_multi_launches'), e.counter('mask_grow_global_launches')) == (n_m + 1, n_g)
            e.set_option('mask_grow', 'global')
            glob = e.masks_from_scoremap(sm, K, keep=keep)
            assert (e.counter('mask_grow_multi_launches'), e.counter('mask_grow_global_launches')) == (n_m + 2, n_g + 1)
        finally:
            e.set_option('mask_grow', 'auto')
        for k in KEEP_KEYS:
            assert np.array_equal(lds[k], got[k]) and np.array_equal(glob[k], got[k]), k
    return got


RECTS5 = [(10, 30, 10, 40, 3.0), (10, 40, 70, 90, 5.0), (60, 100, 20, 50, 4.0), (70, 90, 90, 120, 2.0), (100, 118, 130, 158, 6.0)]


def rect_center(r):
    return 0.5 * (r[0] + r[1] - 1), 0.5 * (r[2] + r[3] - 1)


def run_claim_cases(e, H=120, W=160, both_forms=True):
    """The engineered cases of the claim rule on rect_scoremap maps of H x W (rectangles as for 120 x 160, placed at the same pixels)."""
    chk = lambda sm, K, keep, area=0: assert_keep_exact(e, sm, K, keep, area, both_forms)
    order = sorted(RECTS5, key=lambda r: -r[4])          # discovery order: 6.0, 5.0, 4.0, 3.0, 2.0
    sm5 = HO.rect_scoremap(RECTS5, H, W)
    # no keeps: hp3d_masks_from_scoremap
    for K in (1, 2, 4):
        got = chk(sm5, K, as_keep(K, {}))
        plain = e.masks_from_scoremap(sm5, K)
        for k in HO.MASK_KEYS:
            assert np.array_equal(got[k], plain[k]), k
        assert not got['claimed'].any()
    # slot 0 kept on the highest-scoring rectangle (scale 10: half = 12.8 px): it is claimed, the next one fills slot 1
    r0, c0 = rect_center(order[0])
    got = chk(sm5, 2, as_keep(2, {0: (r0, c0, 10.0)}))
    assert got['claimed'][0].tolist() == [1, 0] and got['valid'][0].tolist() == [0, 1]
    assert got['seed'][0, 1].tolist() == [order[1][0], order[1][2]] and got['seed'][0, 0].tolist() == [-1, -1]
    # ... kept in slot 1: the next object goes to slot 0, the lowest free one
    got = chk(sm5, 3, as_keep(3, {1: (r0, c0, 10.0)}))
    assert got['claimed'][0].tolist() == [0, 1, 0] and got['valid'][0].tolist() == [1, 0, 1]
    assert got['seed'][0, 0].tolist() == [order[1][0], order[1][2]] and got['seed'][0, 2].tolist() == [order[2][0], order[2][2]]
    # second clause: a large object (rows 20..99, cols 20..139, centre (59.5, 79.5)); the kept box sits in its corner at scale 10:
    # the object's centre is 30 / 50 px away (> 12.8) while the slot's centre lies inside the bounding box
    big = HO.rect_scoremap([(20, 100, 20, 140, 4.0), (108, 118, 0, 8, 2.0)], H, W)
    keep = as_keep(2, {0: (28.0, 28.0, 10.0)})
    obj = np.zeros((H, W), F32); obj[20:100, 20:140] = 1
    assert claim_clauses(obj, (28.0, 28.0), 10.0) == (False, True)
    got = chk(big, 2, keep)
    assert got['claimed'][0].tolist() == [1, 0] and got['area'][0].tolist() == [0, 80] and got['valid'][0].tolist() == [0, 1]
    # one object claimed by two kept slots: it counts for the lower one
    got = chk(sm5, 3, as_keep(3, {0: (r0, c0, 10.0), 2: (r0 + 2.0, c0 - 3.0, 8.0)}))
    assert got['claimed'][0].tolist() == [1, 0, 0] and got['valid'][0].tolist() == [0, 1, 0]
    # all slots kept: nothing is reported; the growth runs to the end of the map or the cap and the claims are counted
    r1, c1 = rect_center(order[1])
    got = chk(sm5, 2, as_keep(2, {0: (r0, c0, 10.0), 1: (r1, c1, 10.0)}))
    assert got['claimed'][0].tolist() == [1, 1] and not got['valid'].any() and not got['mask'].any() and np.all(got['seed'] == -1)
    # keeps with an empty det: every free slot absent, nothing claimed
    for mode in ('inf', 'fltmax'):
        G_saved = G.EMPTY_REDUCE
        G.EMPTY_REDUCE = mode
        e.set_option('empty_reduce', mode)
        try:
            empty = HO.rect_scoremap([], H, W)
            got = chk(empty, 3, as_keep(3, {1: (60.0, 80.0, 2.0)}))
            assert not got['valid'].any() and not got['claimed'].any() and np.all(got['seed'] == -1)
            assert np.all(got['center'] == (160.0 if mode == 'inf' else 0.0)) and np.all(got['crop_size'] == 100.0)
            # ... and without keeps the empty map is masks_from_scoremap's (slot 0 reports the global arg-max as its seed)
            got = chk(synth.blob_scoremap('empty'), 2, as_keep(2, {}))
            plain = e.masks_from_scoremap(synth.blob_scoremap('empty'), 2)
            for k in HO.MASK_KEYS:
                assert np.array_equal(got[k], plain[k]), (mode, k)
            assert got['seed'][0, 0, 0] >= 0
        finally:
            G.EMPTY_REDUCE = G_saved
            e.set_option('empty_reduce', 'inf')
    # specks with hands_min_area: a claimed speck is not tested against it but counts toward the cap of 4 K growths.  K = 2, slot 0
    # kept on speck 0 (2 x 2 px, claimed), min_area = 10: 8 growths = speck 0 (claimed), specks 1..4 (dropped), the hand (accepted)
    specks = [(5 + 20 * i, 7 + 20 * i, 5 + 25 * i, 7 + 25 * i, 9.0 - i) for i in range(5)]
    smk = HO.rect_scoremap(specks + [(90, 115, 10, 40, 3.0)], H, W)
    e.set_option('hands_min_area', '10')
    try:
        got = chk(smk, 2, as_keep(2, {0: (5.5, 5.5, 10.0)}), 10)
        assert got['claimed'][0].tolist() == [1, 0] and got['valid'][0].tolist() == [0, 1] and got['area'][0, 1] == 25 * 30
        # K = 1 with its slot kept on the hand itself: 4 growths, all specks, nothing claimed within the cap
        got = chk(smk, 1, as_keep(1, {0: (102.0, 24.5, 5.0)}), 10)
        assert got['claimed'][0].tolist() == [0] and got['valid'][0].tolist() == [0]
        # K = 2, slot 1 kept far from everything: 8 growths, the hand is the sixth and goes to slot 0
        got = chk(smk, 2, as_keep(2, {1: (60.0, 150.0, 10.0)}), 10)
        assert got['claimed'][0].tolist() == [0, 0] and got['valid'][0].tolist() == [1, 0]
    finally:
        e.set_option('hands_min_area', '0')
    # the serpentine of test_engineered_maps (longer than the pass cap) with slot 0 kept on its first piece: the piece is claimed, the
    # remainder comes back as later objects for the free slots
    det = HO.serpentine(H, W)
    sms = np.zeros((1, H, W, 2), F32)
    sms[0, :, :, 1] = np.where(det > 0, 2.0, -2.0)
    sms[0, 0, 0, 1] = 3.0
    first = e.masks_from_scoremap(sms, 1)
    keep = as_keep(4, {0: (float(first['center'][0, 0, 0]), float(first['center'][0, 0, 1]), float(first['scale'][0, 0]))})
    got = chk(sms, 4, keep)
    assert got['claimed'][0, 0] >= 1 and got['valid'][0, 0] == 0
    m = got['mask'][0]
    assert m.sum(axis=0).max() <= 1 and np.all(m.sum(axis=0) <= det) and not np.any(m * first['mask'][0, 0])


def run_random_keeps(e, trials=6, H=96, W=128, both_forms=True):
    """Random rectangles with random keeps: exact against the rule; reported masks are pairwise disjoint and subsets of det; no
    reported object satisfies the claim predicate for any kept slot."""
    rng = np.random.default_rng(13)
    K = 4
    for trial in range(trials):
        rects = []
        for _ in range(int(rng.integers(1, 6))):
            y0, x0 = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 12))
            rects.append((y0, y0 + int(rng.integers(3, 12)), x0, x0 + int(rng.integers(3, 12)), float(rng.uniform(1.0, 6.0))))
        sm = HO.rect_scoremap(rects, H, W)
        kept = {}
        for j in range(K):
            if rng.random() < 0.5:
                r = rects[int(rng.integers(0, len(rects)))]
                cy, cx = rect_center(r)
                kept[j] = (cy + float(rng.uniform(-15, 15)), cx + float(rng.uniform(-15, 15)), float(rng.uniform(2.0, 10.0)))
        keep = as_keep(K, kept)
        got = assert_keep_exact(e, sm, K, keep, both_forms=both_forms)
        det = G.fg_and_detmap(sm)[1][0]
        m = got['mask'][0]
        assert m.sum(axis=0).max() <= 1 and np.all(m <= det[None]), trial
        for j in range(K):
            assert not (got['valid'][0, j] and keep[0][0, j]), trial
            if got['valid'][0, j]:
                assert not any(claims(m[j], keep[1][0, i], keep[2][0, i]) for i in kept), (trial, j)


# ---- the per-slot box rule ---------------------------------------------------------------------------------------------------
def box_rule_slots(kp_hw, valid, box_center, box_scale, H, W, margin=1.25):
    """[B,K,21,2], valid [B,K], the boxes the slots cropped with -> (center [B,K,2], scale [B,K], lost [B,K]): track_oracle.box_rule for
    a valid slot; an absent slot holds its box, lost = 0."""
    B, K = valid.shape
    c, s, lost = TO.box_rule_batch(np.asarray(kp_hw).reshape(B * K, 21, 2), H, W, margin)
    v = np.asarray(valid).reshape(-1) != 0
    c = np.where(v[:, None], c, np.asarray(box_center, F32).reshape(-1, 2))
    s = np.where(v, s, np.asarray(box_scale, F32).reshape(-1))
    lost = np.where(v, lost, 0).astype(np.int32)
    return c.reshape(B, K, 2).astype(F32), s.reshape(B, K).astype(F32), lost.reshape(B, K)


def assert_box_slots(e, kp_hw, valid, box_center, box_scale, H, W, score32=None):
    """hp3d_track_hands_box: valid slots equal hp3d_track_box (and the rule), absent slots hold their box with lost = 0."""
    B, K = valid.shape
    c, s, conf, lost = e.track_hands_box(kp_hw, valid, box_center, box_scale, H, W, score32=score32)
    sc, ss, sconf, slost = e.track_box(kp_hw.reshape(B * K, 21, 2), H, W, score32=None if score32 is None else score32.reshape((B * K,) + score32.shape[2:]))
    v = valid != 0
    assert np.array_equal(c[v], sc.reshape(B, K, 2)[v]) and np.array_equal(s[v], ss.reshape(B, K)[v]) and np.array_equal(lost[v], slost.reshape(B, K)[v])
    assert np.array_equal(conf, sconf.reshape(B, K))          # reported for absent slots as well
    assert np.array_equal(c[~v], box_center[~v]) and np.array_equal(s[~v], box_scale[~v]) and not lost[~v].any()
    rc, rs, rl = box_rule_slots(kp_hw, valid, box_center, box_scale, H, W)
    assert np.array_equal(c, rc) and np.array_equal(s, rs) and np.array_equal(lost, rl)
    if score32 is not None:
        assert np.array_equal(conf.reshape(-1), TO.confidence(score32.reshape((B * K,) + score32.shape[2:])))
    return c, s, conf, lost


# ---- the state machine -------------------------------------------------------------------------------------------------------
FALLBACK_SCALE = F32(256.0) / (F32(100.0) * F32(1.25))


def fallback_center():
    return F32(160.0) if G.EMPTY_REDUCE == 'inf' else F32(0.0)


class Machine(object):
    """The host side of the tracker restated: which step detects, what it keeps, and what the state is afterwards -- fed with the
    device's own score map (detect steps) and keypoints (every step)."""

    def __init__(self, redetect=0, min_area=0, margin=1.25):
        self.redetect, self.min_area, self.margin = redetect, min_area, margin
        self.reset()

    def reset(self):
        self.shape = None
        self.since = 0

    def seed(self, center, scale, valid, H, W):
        B, K = valid.shape
        v = np.asarray(valid) != 0
        self.center = np.where(v[..., None], np.asarray(center, F32), fallback_center()).astype(F32)
        self.scale = np.where(v, np.asarray(scale, F32), FALLBACK_SCALE).astype(F32)
        self.valid, self.lost = v.astype(np.int32), np.zeros((B, K), np.int32)
        self.shape = (B, K, H, W)
        self.since = 0

    def kind(self, B, K, H, W):
        """-> (detect, keep [B,K])."""
        fresh = self.shape != (B, K, H, W)
        if fresh:
            return True, np.zeros((B, K), np.int32)
        v, lost = self.valid != 0, self.lost != 0
        sched = self.redetect > 0 and self.since + 1 >= self.redetect
        detect = bool(np.any(v & lost)) or bool(np.any(~v.any(axis=1))) or sched
        return detect, (v & ~lost).astype(np.int32)

    def boxes(self, B, K, H, W, scoremap=None):
        """The boxes this step crops with and its valid / detected / area / claimed; scoremap [B,H,W,2] (the device's own) on a detect
        step."""
        detect, keep = self.kind(B, K, H, W)
        z = np.zeros((B, K), np.int32)
        if not detect:
            return {'detect': False, 'center': self.center, 'scale': self.scale, 'valid': self.valid, 'detected': z, 'area': z, 'claimed': z}
        if self.shape != (B, K, H, W):
            self.center, self.scale = np.zeros((B, K, 2), F32), np.ones((B, K), F32)
        r = masks_keep_rule(scoremap, K, keep, self.center, self.scale, self.min_area)
        k = keep != 0
        return {'detect': True, 'center': np.where(k[..., None], self.center, r['center']).astype(F32),
                'scale': np.where(k, self.scale, r['scale']).astype(F32), 'valid': np.where(k, 1, r['valid']).astype(np.int32),
                'detected': np.where(k, 0, r['valid']).astype(np.int32), 'area': np.where(k, 0, r['valid'] * r['area']).astype(np.int32),
                'claimed': r['claimed']}

    def advance(self, step, kp_hw, B, K, H, W):
        """After a step that used `step` (from boxes()) and found kp_hw [B,K,21,2]: the next state.  Returns the expected lost flags."""
        c, s, lost = box_rule_slots(kp_hw, step['valid'], step['center'], step['scale'], H, W, self.margin)
        self.center, self.scale, self.valid, self.lost = c, s, step['valid'].copy(), lost
        self.shape = (B, K, H, W)
        self.since = 0 if step['detect'] else self.since + 1
        return lost


STEP_KEYS = ('center', 'scale', 'valid', 'detected', 'area', 'claimed')


def compose_slots(e, frame, hs, o, H, W):
    """Every output of step `o` equals the chain of per-op calls at batch B * K on its boxes, with no tolerance; the next boxes'
    confidence and lost flags are hp3d_track_hands_box's on the device's own keypoints and score maps."""
    B, K = o['scale'].shape
    c, s = o['center'].reshape(-1, 2), o['scale'].reshape(-1)
    comp = TO.compose(e, np.repeat(frame, K, axis=0), hs.reshape(-1, 2), c, s)
    for k in ('crop', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw'):
        if o.get(k) is None:
            continue
        assert np.array_equal(o[k].reshape(comp[k].shape), comp[k]), k
    nc, ns, conf, lost = e.track_hands_box(o['kp_hw'], o['valid'], o['center'], o['scale'], H, W, score32=comp['sm'].reshape(B, K, 32, 32, 21))
    assert np.array_equal(o['confidence'], conf) and np.array_equal(o['lost'], lost)
    assert np.array_equal(conf.reshape(-1), TO.confidence(comp['sm']))
    return nc, ns


def no_seg_rows(e):
    return not [r for r in e.profile() if r[0].startswith('HandSegNet/') or r[0] in ('seg_upsample_softmax', 'mask_grow', 'mask_grow_multi')]


def step_and_check(e, m, frame, hs, K, u8=None, scoremap=None, want_kpmap=True, compose=True):
    """One engine step against the restated machine `m`.  frame: the float32 frame (what the engine sees, also for u8 steps);
    scoremap: e.handsegnet(frame) if the caller has it (computed here on a detect step otherwise).  Returns (outputs, detect)."""
    B, H, W, _ = frame.shape
    detect, _ = m.kind(B, K, H, W)
    nd, nt = e.counter('track_hands_detect_steps'), e.counter('track_hands_tracked_steps')
    e.set_profiling(1)
    try:
        o = e.track_hands_step_u8(u8, hs, K, want_kpmap=want_kpmap) if u8 is not None else e.track_hands_step(frame, hs, K, want_kpmap=want_kpmap)
        rows = [r[0] for r in e.profile()]
        seg_free = no_seg_rows(e)
    finally:
        e.set_profiling(0)
    assert (e.counter('track_hands_detect_steps') - nd, e.counter('track_hands_tracked_steps') - nt) == (int(detect), int(not detect))
    assert seg_free == (not detect) and ('track_hands_select' in rows) == detect and 'track_hands_box' in rows
    if detect and scoremap is None:
        scoremap = e.handsegnet(frame)
    exp = m.boxes(B, K, H, W, scoremap)
    for k in STEP_KEYS:
        assert np.array_equal(o[k], exp[k]), (k, o[k].tolist() if o[k].size < 64 else None, exp[k].tolist() if exp[k].size < 64 else None)
    assert np.array_equal(o['crop'].reshape(B * K, 256, 256, 3),
                          G.crop_image_from_xy(np.repeat(frame, K, axis=0), o['center'].reshape(-1, 2), 256, o['scale'].reshape(-1)))
    if compose:
        compose_slots(e, frame, hs, o, H, W)
    lost = m.advance(exp, o['kp_hw'], B, K, H, W)
    assert np.array_equal(o['lost'], lost)
    for k, v in o.items():
        if v is not None and v.dtype.kind == 'f':
            assert np.all(np.isfinite(v)), k
    return o, detect


def reseed_if_lost(e, m, o, H, W):
    """Random-weight keypoints lose hands on most steps; to reach a tracked step the lost slots are re-seeded with the boxes their own
    keypoints gave (what a tracked step would have used), as track_oracle.run_three_steps(reseed_lost=True) does."""
    v = o['valid'].copy()
    v[:, 0] = 1              # (every image needs a valid slot; an absent slot 0 is seeded on its fall-back box)
    e.track_hands_seed(m.center, m.scale, v, H, W)
    m.seed(m.center, m.scale, v, H, W)


def run_steps(e, weights, B, K, H, W, seed=7, u8=False, oracle_slots=(), steps=3, compose=True, expect_global=False, reseed=True):
    """`steps` steps: step 0 detects and equals hp3d_infer_hands on every shared output; later steps equal the restated machine fed with
    the device's own keypoints and score map, and the chain of per-op calls; sampled slots against the oracle stage by stage.
    Returns the number of tracked steps."""
    hs = HO.hand_sides(B, K)
    e.track_hands_reset()
    m = Machine()
    tracked = 0
    for t in range(steps):
        fr = TO.frames(seed, t, B, H, W)
        fu8 = TO.to_u8(fr) if u8 else None
        if u8:
            fr = G.preprocess_u8(fu8, H, W)
        if t > 0 and reseed and m.kind(B, K, H, W)[0]:
            reseed_if_lost(e, m, o, H, W)
        nu, ng = e.counter('crop_u8_launches'), e.counter('mask_grow_global_launches')
        o, detect = step_and_check(e, m, fr, hs, K, u8=fu8, compose=compose)
        assert (e.counter('mask_grow_global_launches') > ng) == (detect and expect_global)
        if t == 0:
            assert detect
            full = e.infer_hands(fr, hs, K)
            for k in ('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw', 'valid', 'area'):
                assert np.array_equal(o[k], full[k]), k
            assert np.array_equal(o['detected'], full['valid']) and not o['claimed'].any()
        elif not detect:
            tracked += 1
            assert not o['detected'].any() and not o['area'].any()
            if u8:
                assert e.counter('crop_u8_launches') > nu
        if weights is not None and oracle_slots:
            HO.assert_vs_oracle(o, fr, hs, weights, oracle_slots)
    return tracked
