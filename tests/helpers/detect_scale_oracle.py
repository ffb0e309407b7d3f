"""NumPy restatement of detection on a reduced frame (option "detect_scale" = f) -- rule 1 (the detection frame), rule 3
(a detection-frame box in frame coordinates) and rule 4 (a kept slot's frame box in detection-frame coordinates), float32 op by op --
and the checks the CPU (interpreter) and GPU tests share.  Built on oracle.general (scale_from_crop_size, preprocess_u8's operation
order) and, for the multi-hand tracker, on track_hands_oracle's state machine with rules 3 and 4 wrapped around its detection."""
import numpy as np

import track_hands_oracle as THO
import track_oracle as TO
from oracle import general as G

F32 = np.float32
COUNTERS = ('mask_grow_global_launches', 'mask_grow_multi_launches', 'conv_first_launches', 'first_touch_launches', 'lift_fused_launches',
            'conv_wino4_launches', 'conv_wino4_tail_launches', 'conv_wino2_launches', 'conv_wino_launches', 'conv_wino7_launches',
            'conv_wino7_split_launches', 'conv_pw2_launches', 'conv_mfma_launches', 'conv_splitk_reduce_launches', 'conv_h16_launches',
            'fc_tail_launches', 'conv_s2_gemm_launches', 'track_detect_steps', 'track_tracked_steps', 'track_hands_detect_steps',
            'track_hands_tracked_steps', 'crop_u8_launches', 'detect_scale_steps')


def detect_shape(H, W, f):
    return -(-H // f), -(-W // f)


def _window_counts(H, W, f):
    Hd, Wd = detect_shape(H, W, f)
    ny = np.minimum(f, H - np.arange(Hd) * f)
    nx = np.minimum(f, W - np.arange(Wd) * f)
    return (ny[:, None] * nx[None, :]).astype(F32)[None, :, :, None]


def _window_sum(x, f, dtype):
    """Rows outer, columns inner, one addition of `dtype` per source pixel; positions outside the frame are skipped."""
    B, H, W, C = x.shape
    Hd, Wd = detect_shape(H, W, f)
    acc = np.zeros((B, Hd, Wd, C), dtype)
    for dy in range(f):
        for dx in range(f):
            sub = x[:, dy::f, dx::f, :].astype(dtype)
            acc[:, :sub.shape[1], :sub.shape[2]] = (acc[:, :sub.shape[1], :sub.shape[2]] + sub).astype(dtype)
    return acc


def downscale(image, f):
    """Rule 1, float32 frames [B,H,W,3]: the clipped f x f window as a sequential float32 sum in row-major order, / float32(n)."""
    x = np.asarray(image, F32)
    return (_window_sum(x, f, F32) / _window_counts(x.shape[1], x.shape[2], f)).astype(F32)


def downscale_u8(image_u8, f):
    """Rule 1, uint8 frames: the exact integer sum, then (float32(sum) / float32(n)) / 255 - 0.5 in oracle.general.preprocess_u8's order."""
    x = np.asarray(image_u8)
    assert x.dtype == np.uint8
    mean = (_window_sum(x, f, np.int64).astype(F32) / _window_counts(x.shape[1], x.shape[2], f)).astype(F32)
    return (mean / F32(255.0) - F32(0.5)).astype(F32)


def boxes_to_frame(center_d, crop_size_d, f):
    """Rule 3: (centre_d, crop_size_d) of the detection frame -> (centre, crop_size, scale) of the frame."""
    with np.errstate(invalid='ignore', over='ignore'):
        center = (np.asarray(center_d, F32) * F32(f) + F32((f - 1) / 2)).astype(F32)
        size = (np.asarray(crop_size_d, F32) * F32(f)).astype(F32)
        return center, size, G.scale_from_crop_size(size)


def boxes_to_detect(center, scale, f):
    """Rule 4: a kept slot's frame box -> (centre_d, scale_d) for the claim rule on the detection frame."""
    with np.errstate(invalid='ignore', over='ignore'):
        return ((np.asarray(center, F32) - F32((f - 1) / 2)) / F32(f)).astype(F32), (np.asarray(scale, F32) * F32(f)).astype(F32)


DOWNSCALE_SHAPES = [(3, 37, 53, 2), (2, 50, 70, 3), (1, 64, 48, 4), (1, 33, 130, 8)]
# ... and rows that take the one-load form at each f (row pitch a multiple of the load's alignment) with ragged last rows / columns
DOWNSCALE_SHAPES_WIDE = [(2, 19, 38, 2), (1, 18, 44, 4), (2, 20, 36, 8), (1, 17, 72, 8), (1, 16, 16, 1)]


def assert_downscale_exact(e, B, H, W, f):
    rng = np.random.default_rng(H * 1000 + W + f)
    x = rng.uniform(-0.5, 0.5, (B, H, W, 3)).astype(F32)
    x[0, :2, :3] *= F32(1e4)             # (a sum whose order matters)
    got = e.downscale(x, f)
    assert got.shape == (B,) + detect_shape(H, W, f) + (3,) and np.array_equal(got, downscale(x, f))
    u8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    got = e.downscale_u8(u8, f)
    assert got.dtype == F32 and np.array_equal(got, downscale_u8(u8, f))
    for v, r in ((255, 0.5), (0, -0.5)):
        assert np.all(e.downscale_u8(np.full((B, H, W, 3), v, np.uint8), f) == F32(r)), v


def box_cases(f, rng):
    """64 random boxes, both empty_reduce fall-back boxes and a NaN centre: (center_d [n,2], crop_size_d [n])."""
    c = np.concatenate([rng.uniform(-20, 700, (64, 2)), [[160.0, 160.0], [0.0, 0.0], [np.nan, 12.0]]]).astype(F32)
    s = np.concatenate([rng.uniform(0.0, 400, 64), [100.0, 100.0, 30.0]]).astype(F32)
    s[:3] = (0.0, 1.0, 1000.0)          # both clamps of the scale
    return c, s


def assert_boxes_exact(e, f):
    rng = np.random.default_rng(f)
    c_d, s_d = box_cases(f, rng)
    c, s, sc = e.boxes_to_frame(c_d, s_d, f)
    rc, rs, rsc = boxes_to_frame(c_d, s_d, f)
    assert np.array_equal(c, rc, equal_nan=True) and np.array_equal(s, rs) and np.array_equal(sc, rsc)
    assert np.isnan(c[-1, 0]) and c[-1, 1] == F32(12 * f) + F32((f - 1) / 2) and np.isnan(c).sum() == 1
    assert sc[0] == 5 and sc[2] == 0.25 and np.all(sc[64:66] == G.scale_from_crop_size(F32(100 * f)))
    assert np.all(c[64] == F32(160 * f) + F32((f - 1) / 2)) and np.all(c[65] == F32((f - 1) / 2))
    # rule 4 on frame boxes (scales as the trackers hold them), the NaN centre included
    ks = rng.uniform(0.25, 10.0, len(s_d)).astype(F32)
    cd, sd = e.boxes_to_detect(c, ks, f)
    rcd, rsd = boxes_to_detect(c, ks, f)
    assert np.array_equal(cd, rcd, equal_nan=True) and np.array_equal(sd, rsd) and np.isnan(cd).sum() == 1
    # the centre of a detection pixel goes to the centre of its window and back
    p = np.arange(64, dtype=F32).reshape(32, 2)
    assert np.array_equal(boxes_to_detect(boxes_to_frame(p, np.ones(32, F32), f)[0], np.ones(32, F32), f)[0], p)


def run_detect_step(e, step):
    """Runs `step()` with profiling on; returns (outputs, profile row names, counter deltas)."""
    n0 = {k: e.counter(k) for k in COUNTERS}
    e.set_profiling(1)
    try:
        o = step()
        rows = [r[0] for r in e.profile()]
    finally:
        e.set_profiling(0)
    return o, rows, {k: e.counter(k) - n0[k] for k in COUNTERS}


def assert_detect_step_is_composition(e, o, rows, frame, f, u8=None):
    """One detect step `o` of hp3d_track_step* at detect_scale f (fresh state: every image takes the detected box) against the
    composition of the engine's own per-op calls -- downscale -> handsegnet at (Hd, Wd) -> mask_from_scoremap -> rule 3 (this file's)
    -> crop_and_resize on the full frame -- bit for bit.  frame: float32, what the crop sees (the normalised frame for a uint8 step)."""
    src = e.downscale_u8(u8, f) if u8 is not None else e.downscale(frame, f)
    _, c_d, size_d, _, _ = e.mask_from_scoremap(e.handsegnet(src))
    center, _, scale = boxes_to_frame(c_d, size_d, f)
    assert np.all(o['detected'] == 1)
    assert np.array_equal(o['center'], center) and np.array_equal(o['scale'], scale)
    crop = e.crop_and_resize_u8(u8, center, scale, 256) if u8 is not None else e.crop_and_resize(frame, center, scale, 256)
    assert np.array_equal(o['crop'], crop)
    assert np.array_equal(crop, G.crop_image_from_xy(frame, center, 256, scale))
    assert rows.count('downscale_u8' if u8 is not None else 'downscale') == 1 and rows.count('box_to_frame') == 1
    assert 'preprocess_u8' not in rows and 'box_to_detect' not in rows
    if u8 is not None:
        assert rows.count('crop_and_resize_u8') == 1 and 'crop_and_resize' not in rows and 'downscale' not in rows
    else:
        assert rows.count('crop_and_resize') == 1 and 'crop_and_resize_u8' not in rows
    assert rows.index('box_to_frame') < rows.index('track_select')


# ---- the claim rule at f: track_hands_oracle on detection-frame quantities, rules 3 and 4 around it ------------------------------------
def masks_keep_rule_at(scoremap_d, K, keep, center, scale, f, min_area=0):
    """scoremap_d [B,Hd,Wd,2] (the detection frame's), keep [B,K] and the kept slots' FRAME boxes -> track_hands_oracle.masks_keep_rule
    on the detection frame with the boxes of rule 4, its boxes mapped by rule 3."""
    kc_d, ks_d = boxes_to_detect(center, scale, f)
    r = THO.masks_keep_rule(scoremap_d, K, keep, kc_d, ks_d, min_area)
    r['center'], r['crop_size'], r['scale'] = boxes_to_frame(r['center'], r['crop_size'], f)
    return r


def run_claim_at(e, f=2, Hd=60, Wd=80):
    """Two blobs on the detection frame and one kept slot whose frame box, mapped by rule 4, claims blob 0 and not blob 1: the first
    clause with half = 128 / (scale * f) detection pixels.  The same frame box read as a detection-frame box would not claim."""
    import hands_oracle as HO
    K = 2
    rects = [(10, 20, 10, 22, 5.0), (40, 52, 50, 66, 3.0)]          # blob 0 (found first), blob 1
    sm = HO.rect_scoremap(rects, Hd, Wd)
    r0, c0 = THO.rect_center(rects[0])
    # the kept slot sits 6 frame pixels beside blob 0's centre in frame coordinates, scale 10 (half = 12.8 frame = 6.4 detection pixels)
    fc = boxes_to_frame(np.array([[r0, c0]], F32), np.ones(1, F32), f)[0][0] + F32(6.0)
    keep, kc, ks = THO.as_keep(K, {0: (float(fc[0]), float(fc[1]), 10.0)})
    kc_d, ks_d = e.boxes_to_detect(kc, ks, f)
    rcd, rsd = boxes_to_detect(kc, ks, f)
    assert np.array_equal(kc_d, rcd) and np.array_equal(ks_d, rsd)
    obj0 = np.zeros((Hd, Wd), F32); obj0[10:20, 10:22] = 1
    obj1 = np.zeros((Hd, Wd), F32); obj1[40:52, 50:66] = 1
    assert THO.claims(obj0, kc_d[0, 0], ks_d[0, 0]) and not THO.claims(obj1, kc_d[0, 0], ks_d[0, 0])
    assert not THO.claims(obj0, kc[0, 0], ks[0, 0])                 # (unmapped, the box lies elsewhere)
    got = e.masks_from_scoremap(sm, K, keep=(keep, kc_d, ks_d))
    got['center'], got['crop_size'], got['scale'] = e.boxes_to_frame(got['center'], got['crop_size'], f)
    ref = masks_keep_rule_at(sm, K, keep, kc, ks, f)
    for k in ('claimed', 'valid', 'area', 'seed', 'center', 'crop_size', 'scale'):
        assert np.array_equal(got[k], ref[k]), (k, got[k].tolist(), ref[k].tolist())
    assert got['claimed'][0].tolist() == [1, 0] and got['valid'][0].tolist() == [0, 1]
    assert got['seed'][0, 1].tolist() == [40, 50] and got['area'][0, 1] == 12 * 16
    assert np.array_equal(got['center'][0, 1], boxes_to_frame(np.array(THO.rect_center(rects[1]), F32), F32(15.0), f)[0])
    return got


class MachineAt(THO.Machine):
    """track_hands_oracle's state machine at detect_scale f: the state is in frame coordinates; a detect step maps the kept boxes to the
    detection frame (rule 4), runs the claimed detection on the device's own detection-frame score map and maps its boxes back (rule 3).
    A change of f counts as a change of shape."""

    def __init__(self, f, **kw):
        self.f = f
        THO.Machine.__init__(self, **kw)

    def boxes(self, B, K, H, W, scoremap=None):
        detect, keep = self.kind(B, K, H, W)
        if not detect:
            return THO.Machine.boxes(self, B, K, H, W)
        z = np.zeros((B, K), np.int32)
        if self.shape != (B, K, H, W):
            self.center, self.scale = np.zeros((B, K, 2), F32), np.ones((B, K), F32)
        r = masks_keep_rule_at(scoremap, K, keep, self.center, self.scale, self.f, self.min_area)
        k = keep != 0
        return {'detect': True, 'center': np.where(k[..., None], self.center, r['center']).astype(F32),
                'scale': np.where(k, self.scale, r['scale']).astype(F32), 'valid': np.where(k, 1, r['valid']).astype(np.int32),
                'detected': np.where(k, 0, r['valid']).astype(np.int32), 'area': np.where(k, 0, r['valid'] * r['area']).astype(np.int32),
                'claimed': r['claimed']}


def step_hands_and_check(e, m, frame, hs, K):
    """One hp3d_track_hands_step at detect_scale m.f against MachineAt, bit for bit.  Returns (outputs, detect, profile rows)."""
    B, H, W, _ = frame.shape
    detect, keep = m.kind(B, K, H, W)
    o, rows, dn = run_detect_step(e, lambda: e.track_hands_step(frame, hs, K))
    assert (dn['track_hands_detect_steps'], dn['track_hands_tracked_steps'], dn['detect_scale_steps']) == (int(detect), int(not detect), int(detect))
    for name in ('downscale', 'box_to_frame', 'box_to_detect', 'mask_grow_multi', 'track_hands_select'):
        assert rows.count(name) == int(detect), (name, rows)
    exp = m.boxes(B, K, H, W, e.handsegnet(e.downscale(frame, m.f)) if detect else None)
    for k in THO.STEP_KEYS:
        assert np.array_equal(o[k], exp[k]), (k, o[k].tolist(), exp[k].tolist())
    assert np.array_equal(o['crop'].reshape(B * K, 256, 256, 3),
                          G.crop_image_from_xy(np.repeat(frame, K, axis=0), o['center'].reshape(-1, 2), 256, o['scale'].reshape(-1)))
    lost = m.advance(exp, o['kp_hw'], B, K, H, W)
    assert np.array_equal(o['lost'], lost)
    return o, detect, rows
