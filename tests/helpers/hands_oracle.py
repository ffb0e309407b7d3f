"""NumPy restatement of the multi-hand rule with oracle.general's functions, and the checks the CPU (interpreter)
and GPU multi-hand tests share.

The rule, for one image with fg, det = fg_and_detmap(scoremap), grow = grow_objectmap (21x21 dilation, pass cap max(H, W) // 10):
R = det; the next object grows inside R from the first arg-max (row-major) of fg over R's pixels and is taken out of R; an object of
at least min_area pixels is the next hand; at most 4 K objects are grown per image (the cap holds for the image: a growth is never
started once 4 K have run, whether the last one was accepted or not).  Where det is empty, slot 0 is the single-hand result (seed =
the global arg-max, empty mask, fall-back box) with valid = 0.  Absent slots: zero mask, seed (-1, -1), valid = area = 0, fall-back box."""
import numpy as np

from hand3d_amd import synth
from hand3d_amd.utils import general as PG
from oracle import general as G
from oracle import nets as N
from oracle import tf_ops as T

F32 = np.float32
TOL_HEATMAP = 1e-3          # the project's full-path gates
TOL_KP3D = 1e-4
MASK_KEYS = ('mask', 'center', 'crop_size', 'scale', 'seed', 'valid', 'area')


def hands_rule(scoremap, K, min_area=0):
    """scoremap [H,W,2] -> list of K dicts (mask [H,W] f32, seed int32 [2], valid, area)."""
    fg, det = G.fg_and_detmap(np.asarray(scoremap, F32)[None])
    fg, det = fg[0], det[0]
    H, W = det.shape
    slots = []
    if not det.any():
        seed = G.find_max_location(fg[None])[0]
        obj, _ = G.grow_objectmap(det, seed, early_exit=True)
        slots.append({'mask': obj, 'seed': seed.astype(np.int32), 'valid': 0, 'area': int(obj.sum())})
    else:
        R = det.copy()
        tries = 0
        while len(slots) < K and tries < 4 * K and R.any():
            idx = int(np.argmax(np.where(R == 1, fg, -np.inf)))          # first maximum of the row-major flattened map
            seed = np.array([idx // W, idx % W], np.int32)
            obj, _ = G.grow_objectmap(R, seed, early_exit=True)
            R = (R * (1 - obj)).astype(F32)
            tries += 1
            if int(obj.sum()) >= min_area:
                slots.append({'mask': obj, 'seed': seed, 'valid': 1, 'area': int(obj.sum())})
    while len(slots) < K:
        slots.append({'mask': np.zeros((H, W), F32), 'seed': np.array([-1, -1], np.int32), 'valid': 0, 'area': 0})
    return slots


def masks_rule(scoremap, K, min_area=0):
    """scoremap [B,H,W,2] -> dict like Engine.masks_from_scoremap's."""
    sm = np.asarray(scoremap, F32)
    B, H, W, _ = sm.shape
    o = {'mask': np.zeros((B, K, H, W), F32), 'center': np.zeros((B, K, 2), F32), 'crop_size': np.zeros((B, K), F32),
         'scale': np.zeros((B, K), F32), 'seed': np.zeros((B, K, 2), np.int32), 'valid': np.zeros((B, K), np.int32),
         'area': np.zeros((B, K), np.int32)}
    for b in range(B):
        for j, s in enumerate(hands_rule(sm[b], K, min_area)):
            center, _, size = G.calc_center_bb(s['mask'][None, :, :, None])
            o['mask'][b, j] = s['mask']
            o['center'][b, j] = center[0]
            o['crop_size'][b, j] = size[0, 0]
            o['scale'][b, j] = G.scale_from_crop_size(size)[0, 0]
            o['seed'][b, j] = s['seed']
            o['valid'][b, j] = s['valid']
            o['area'][b, j] = s['area']
    return o


def assert_masks_exact(e, sm, K, min_area=0):
    """The engine's mask stage equals the rule bit for bit (the caller has set option hands_min_area to min_area)."""
    got = e.masks_from_scoremap(sm, K)
    ref = masks_rule(sm, K, min_area)
    for k in MASK_KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        assert np.array_equal(got[k], ref[k]), (k, got[k] if got[k].size < 64 else None, ref[k] if ref[k].size < 64 else None)
    return got


def assert_slot0_is_single_hand(e, sm, got):
    """Slot 0 (hands_min_area off) equals hp3d_mask_from_scoremap's hand."""
    mask, center, size, scale, seed = e.mask_from_scoremap(sm)
    assert np.array_equal(got['mask'][:, 0], mask) and np.array_equal(got['center'][:, 0], center)
    assert np.array_equal(got['crop_size'][:, 0], size[:, 0]) and np.array_equal(got['scale'][:, 0], scale[:, 0])
    assert np.array_equal(got['seed'][:, 0], seed)


def assert_lds_equals_global(e, sm, K):
    """Both forms of the kernel give the same bits, and the counters tell them apart."""
    e.set_option('mask_grow', 'lds')
    try:
        n_m, n_g = e.counter('mask_grow_multi_launches'), e.counter('mask_grow_global_launches')
        lds = e.masks_from_scoremap(sm, K)
        assert (e.counter('mask_grow_multi_launches'), e.counter('mask_grow_global_launches')) == (n_m + 1, n_g)
        e.set_option('mask_grow', 'global')
        glob = e.masks_from_scoremap(sm, K)
        assert (e.counter('mask_grow_multi_launches'), e.counter('mask_grow_global_launches')) == (n_m + 2, n_g + 1)
    finally:
        e.set_option('mask_grow', 'auto')
    for k in MASK_KEYS:
        assert np.array_equal(lds[k], glob[k]), k
    return lds


def rect_scoremap(rects, H=120, W=160, background=-2.0):
    """[1,H,W,2] logits: class 0 at 0, class 1 = `background` (fg < 1/2) except rectangles (y0, y1, x0, x1, logit > 0)."""
    sm = np.zeros((1, H, W, 2), F32)
    sm[..., 1] = background
    for (y0, y1, x0, x1, s) in rects:
        sm[0, y0:y1, x0:x1, 1] = s
    return sm


def serpentine(H, W, pitch=12):
    """1-px lines every `pitch` rows joined at alternating ends: the growth advances 10 px per pass along the path."""
    det = np.zeros((H, W), np.uint8)
    rows = list(range(0, H, pitch))
    for i, r in enumerate(rows):
        det[r, :] = 1
        if i + 1 < len(rows):
            c = W - 1 if i % 2 == 0 else 0
            det[r:rows[i + 1] + 1, c] = 1
    return det


def hand_sides(B, K):
    return synth.hand_sides(B * K).reshape(B, K, 2)


def compose(e, frame, hs, center, scale):
    """The chain of existing ops the back half is made of, at batch B * K on the same engine (frame b repeated K times)."""
    B, K = scale.shape
    c, s = center.reshape(-1, 2), scale.reshape(-1)
    crop = e.crop_and_resize(np.repeat(frame, K, axis=0), c, s, 256)
    sm = e.posenet2d(crop)[2]
    coord3d = e.pose3d(sm, hs.reshape(-1, 2))[0]
    kp_crop = e.detect_keypoints(sm)
    kp_hw = np.stack([PG.trafo_coords(kp_crop[i], c[i:i + 1], s[i:i + 1].reshape(1, 1), 256) for i in range(B * K)])
    kpmap = e.resize_bilinear(sm, 256, 256)
    r = {'crop': crop, 'coord3d': coord3d, 'kp_crop': kp_crop, 'kp_hw': kp_hw, 'kpmap': kpmap}
    return {k: v.reshape((B, K) + v.shape[1:]) for k, v in r.items()}


def assert_back_half_is_composition(e, o, frame, hs):
    c = compose(e, frame, hs, o['center'], o['scale'])
    for k in ('crop', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw'):
        if o.get(k) is None:
            continue
        assert np.array_equal(o[k], c[k]), k          # the same kernels at the same shapes: no tolerance


def assert_vs_oracle(o, frame, hs, weights, slots):
    """Stage-wise against the oracle on the device's own boxes / crops (DESIGN.md 2 gates); slots = [(b, j), ...]."""
    for b, j in slots:
        crop = G.crop_image_from_xy(frame[b:b + 1], o['center'][b, j:j + 1], 256, o['scale'][b, j:j + 1])
        assert np.array_equal(o['crop'][b, j:j + 1], crop), (b, j)
        sm32 = N.posenet2d(weights, o['crop'][b, j:j + 1])[-1]
        assert np.abs(o['kpmap'][b, j:j + 1] - T.resize_bilinear_legacy(sm32, 256, 256)).max() < TOL_HEATMAP, (b, j)
        assert np.abs(o['coord3d'][b, j:j + 1] - N.pose3d(weights, sm32, hs[b, j:j + 1])[0]).max() < TOL_KP3D, (b, j)


def check_whole_path(e, frame, K, weights=None, oracle_slots=(), expect_all_valid=True):
    """hp3d_infer_hands at K on `frame` [B,H,W,3]: the mask stage exact on the device's own score map, slot 0 equal to the K = 1 call
    and (through it) to hp3d_infer_full_kp, the back half equal to the chain of per-op calls, optionally the oracle on some slots."""
    B, H, W, _ = frame.shape
    hs = hand_sides(B, K)
    o = e.infer_hands(frame, hs, K, want_mask=True)
    ref = masks_rule(o['scoremap'], K)
    assert np.array_equal(o['mask'], ref['mask']) and np.array_equal(o['center'], ref['center'])
    assert np.array_equal(o['scale'], ref['scale']) and np.array_equal(o['valid'], ref['valid']) and np.array_equal(o['area'], ref['area'])
    if expect_all_valid:
        assert np.all(o['valid'] == 1), o['valid']
    assert np.all(o['area'] == o['mask'].sum(axis=(2, 3)).astype(np.int32))
    o1 = e.infer_hands(frame, hs[:, :1], 1, want_mask=True, outputs=('scale', 'center'))
    assert np.array_equal(o['mask'][:, 0], o1['mask'][:, 0]) and np.array_equal(o['center'][:, 0], o1['center'][:, 0])
    assert np.array_equal(o['scale'][:, 0], o1['scale'][:, 0])
    assert_back_half_is_composition(e, o, frame, hs)
    for v in o.values():
        if v is not None and v.dtype.kind == 'f':
            assert np.all(np.isfinite(v))
    if weights is not None:
        assert_vs_oracle(o, frame, hs, weights, oracle_slots)
    return o


def assert_k1_is_infer_full(e, frame):
    """K = 1: every output of hp3d_infer_hands equals hp3d_infer_full_kp's."""
    B = frame.shape[0]
    hs = synth.hand_sides(B)
    keys = ('scoremap', 'crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw')
    full = e.infer_full(frame, hs, want_mask=True, outputs=keys)
    o = e.infer_hands(frame, hs.reshape(B, 1, 2), 1, want_mask=True)
    assert np.array_equal(o['scoremap'], full['scoremap'])
    for k in keys[1:] + ('mask',):
        assert np.array_equal(o[k].reshape(full[k].shape), full[k]), k
    return o


def background_frame_scoremap_is_empty(o):
    return not G.fg_and_detmap(o['scoremap'])[1].any()
