"""Several hands per frame through the real library: the mask stage bit for bit against the rule
(tests/helpers/hands_oracle.py, shared with the interpreter tests) on engineered maps and both kernel forms, and the whole path --
K = 1 equal to hp3d_infer_full_kp, K = 2 and 4 with the mask stage exact on the device's own score map, slot 0 the single-hand
result, the back half equal to the chain of per-op calls at batch B * K and to the oracle stage by stage -- at 240x320, at 320x320
with B = 8, on one 720x1280 frame (global form) and once with half-precision trunks; the uint8, device-pointer and chunked forms;
an all-background frame; errors, counters and profile rows."""
import os
import sys

import numpy as np
import pytest

from hand3d_amd import synth
from oracle import general as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import hands_oracle as HO      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def eng(gpu_engine, synth_weights):
    gpu_engine.load_weight_dict(synth_weights)
    gpu_engine.finalize_weights(0)
    return gpu_engine


def check_masks(e, sm, K, area=0):
    got = HO.assert_masks_exact(e, sm, K, area)
    both = HO.assert_lds_equals_global(e, sm, K)
    for k in HO.MASK_KEYS:
        assert np.array_equal(got[k], both[k]), k
    if area == 0:
        HO.assert_slot0_is_single_hand(e, sm, got)
    return got


@pytest.mark.parametrize("K", [1, 2, 3])
def test_mask_cases(gpu_engine, monkeypatch, K):
    for case in sorted(synth.MASK_CASES):
        if case == 'empty':
            continue
        got = check_masks(gpu_engine, synth.blob_scoremap(case), K)
        nobj = 2 if case.startswith('two_blobs') else 1          # (gap10 too: see tests/test_hands.py::test_mask_cases)
        assert got['valid'][0].tolist() == [1 if j < nobj else 0 for j in range(K)], case
        if nobj == 2 and K >= 2:
            assert 20 <= got['seed'][0, 0, 1] < 50 and 60 <= got['seed'][0, 1, 1] < 90
    for mode in ('inf', 'fltmax'):
        monkeypatch.setattr(G, 'EMPTY_REDUCE', mode)
        gpu_engine.set_option('empty_reduce', mode)
        try:
            got = check_masks(gpu_engine, synth.blob_scoremap('empty'), K)
            assert not got['valid'].any() and np.all(got['center'] == (160.0 if mode == 'inf' else 0.0))
        finally:
            gpu_engine.set_option('empty_reduce', 'inf')


def test_engineered_maps(gpu_engine):
    e = gpu_engine
    rects = [(10, 30, 10, 40, 3.0), (10, 40, 70, 90, 5.0), (60, 100, 20, 50, 4.0), (70, 90, 90, 120, 2.0), (100, 118, 130, 158, 6.0)]
    for n, K in ((3, 2), (3, 4), (5, 2), (5, 4)):
        got = check_masks(e, HO.rect_scoremap(rects[:n]), K)
        assert got['valid'][0].sum() == min(n, K)
    got = check_masks(e, HO.rect_scoremap([(50, 70, 10, 30, 3.0), (20, 40, 100, 130, 3.0), (21, 30, 40, 60, 3.0)]), 3)
    assert got['seed'][0].tolist() == [[20, 100], [21, 40], [50, 10]]          # ties go to the first pixel
    specks = [(5 + 20 * i, 7 + 20 * i, 5 + 25 * i, 7 + 25 * i, 9.0 - i) for i in range(5)]
    sm = HO.rect_scoremap(specks + [(90, 115, 10, 40, 3.0)])
    e.set_option('hands_min_area', '10')
    try:
        assert check_masks(e, sm, 1, 10)['valid'][0].tolist() == [0]           # four tries, all specks
        assert check_masks(e, sm, 2, 10)['valid'][0].tolist() == [1, 0]        # eight tries: five specks, then the hand
        got = check_masks(e, HO.rect_scoremap([(10, 12, 10, 12, 6.0), (60, 80, 60, 80, 3.0)]), 2, 10)
        assert got['valid'][0].tolist() == [1, 0] and got['seed'][0, 0].tolist() == [60, 60]
    finally:
        e.set_option('hands_min_area', '0')
    # a serpentine longer than the pass cap: hand 0 is the single-hand cut-off mask, the remainder comes back as later hands
    H, W = 120, 160
    det = HO.serpentine(H, W)
    sm = np.zeros((1, H, W, 2), F32)
    sm[0, :, :, 1] = np.where(det > 0, 2.0, -2.0)
    sm[0, 0, 0, 1] = 3.0
    got = check_masks(e, sm, 4)
    assert got['valid'][0].tolist() == [1, 1, 1, 1] and 0 < got['area'][0, 0] < det.sum()
    assert got['mask'][0].sum(axis=0).max() == 1 and np.all(got['mask'][0].sum(axis=0) <= det)


def test_random_rectangles_properties_and_large_frame(gpu_engine):
    rng = np.random.default_rng(5)
    H, W = 96, 128
    for trial in range(8):
        rects = []
        for _ in range(int(rng.integers(1, 5))):
            y0, x0 = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 12))
            rects.append((y0, y0 + int(rng.integers(3, 12)), x0, x0 + int(rng.integers(3, 12)), float(rng.uniform(1.0, 6.0))))
        sm = HO.rect_scoremap(rects, H, W)
        det = G.fg_and_detmap(sm)[1][0]
        m = check_masks(gpu_engine, sm, 4)['mask'][0]
        assert m.sum(axis=0).max() <= 1 and np.all(m <= det[None]) and np.array_equal(m.sum(axis=0), det), trial
    H, W = 540, 960
    y, x = np.mgrid[:H, :W]
    sm = np.zeros((1, H, W, 2), F32)
    sm[..., 1] = -2.0
    for cy, cx, s in ((120, 150, 3.0), (400, 800, 4.0)):
        sm[0, :, :, 1] = np.where(((y - cy) / 45.0) ** 2 + ((x - cx) / 35.0) ** 2 <= 1.0, s, sm[0, :, :, 1])
    n_g = gpu_engine.counter('mask_grow_global_launches')
    got = HO.assert_masks_exact(gpu_engine, sm, 3)
    assert gpu_engine.counter('mask_grow_global_launches') == n_g + 1 and got['valid'][0].tolist() == [1, 1, 0]
    HO.assert_slot0_is_single_hand(gpu_engine, sm, got)


@pytest.mark.parametrize("B", [1, 3])
def test_k1_is_infer_full(eng, B):
    HO.assert_k1_is_infer_full(eng, synth.make_batch(11, B, 240, 320))


@pytest.mark.parametrize("K", [2, 4])
def test_whole_path_240x320(eng, synth_weights, K):
    n = eng.counter('mask_grow_multi_launches')
    o = HO.check_whole_path(eng, synth.make_batch(0, 3, 240, 320), K, synth_weights, oracle_slots=[(0, 0), (1, K - 1)])
    assert eng.counter('mask_grow_multi_launches') == n + 2          # one per call: the K call and the K = 1 call inside the check
    print("K=%d areas %s" % (K, o['area'].tolist()))


def test_whole_path_b8_320(eng, synth_weights):
    HO.check_whole_path(eng, synth.make_batch(40, 8, 320, 320), 4, synth_weights, oracle_slots=[(7, 3)])
    HO.check_whole_path(eng, synth.make_batch(40, 8, 320, 320), 2)


def test_whole_path_720p_global_form(eng, synth_weights):
    ng = eng.counter('mask_grow_global_launches')
    HO.check_whole_path(eng, synth.make_batch(5, 1, 720, 1280), 2, synth_weights, oracle_slots=[(0, 1)])
    assert eng.counter('mask_grow_global_launches') == ng + 2


def test_profile_rows_and_counters(eng):
    fr, hs = synth.make_batch(2, 2, 240, 320), HO.hand_sides(2, 4)
    eng.set_profiling(1)
    try:
        n = eng.counter('mask_grow_multi_launches')
        eng.infer_hands(fr, hs, 4, outputs=('coord3d',))
        rows = [r[0] for r in eng.profile()]
        assert eng.counter('mask_grow_multi_launches') == n + 1
        eng.infer_full(fr, synth.hand_sides(2), outputs=('coord3d',))
        single = [r[0] for r in eng.profile()]
    finally:
        eng.set_profiling(0)
    seg = [r for r in rows if r.startswith('HandSegNet/')]
    assert seg and seg == [r for r in single if r.startswith('HandSegNet/')]          # HandSegNet once per call, whatever K
    assert rows.count('mask_grow_multi') == 1 and 'mask_grow' not in rows and rows.count('crop_and_resize') == 1


def test_chunks_equal_call_by_call(eng):
    """A batch above micro_batch / K runs chunk by chunk (one growth launch per chunk) and equals the same frames call by call."""
    B, K = 5, 2
    fr, hs = synth.make_batch(60, B, 240, 320), HO.hand_sides(B, K)
    eng.set_option('micro_batch', '4')          # 4 / 2 = two frames per chunk: 2 + 2 + 1
    try:
        n = eng.counter('mask_grow_multi_launches')
        o = eng.infer_hands(fr, hs, K, want_mask=True)
        assert eng.counter('mask_grow_multi_launches') == n + 3
        for b0, b1 in ((0, 2), (2, 4), (4, 5)):
            p = eng.infer_hands(fr[b0:b1], hs[b0:b1], K, want_mask=True)
            for k, v in p.items():
                assert np.array_equal(o[k][b0:b1], v), (k, b0)
    finally:
        eng.set_option('micro_batch', 'auto')


def test_u8_and_dev_forms(eng):
    B, H, W, K = 2, 240, 320, 2
    fr, hs = synth.make_batch(70, B, H, W), HO.hand_sides(B, K)
    u8 = np.clip(np.rint((fr + 0.5) * 255.0), 0, 255).astype(np.uint8)
    o8 = eng.infer_hands_u8(u8, hs, K, H=H, W=W, want_mask=True)
    of = eng.infer_hands(eng.preprocess_u8(u8, H, W), hs, K, want_mask=True)
    for k, v in of.items():
        assert np.array_equal(o8[k], v), k
    host = eng.infer_hands(fr, hs, K, want_mask=True)
    shapes = {'scoremap': ((B, H, W, 2), F32), 'crop': ((B, K, 256, 256, 3), F32), 'scale': ((B, K), F32), 'center': ((B, K, 2), F32),
              'kpmap': ((B, K, 256, 256, 21), F32), 'coord3d': ((B, K, 21, 3), F32), 'mask': ((B, K, H, W), F32),
              'kp_crop': ((B, K, 21, 2), np.int32), 'kp_hw': ((B, K, 21, 2), np.float64), 'valid': ((B, K), np.int32),
              'area': ((B, K), np.int32)}
    bufs = {k: eng.dev_alloc(int(np.prod(s)) * np.dtype(dt).itemsize) for k, (s, dt) in shapes.items()}
    d_img, d_hs = eng.to_device(fr), eng.to_device(hs)
    eng.infer_hands_dev(B, H, W, K, d_img, d_hs, **{k: int(v) for k, v in bufs.items()})
    eng.sync()
    for k, (s, dt) in shapes.items():
        assert np.array_equal(eng.to_host(bufs[k], s, dt), host[k]), k
    for b in list(bufs.values()) + [d_img, d_hs]:
        b.free()


def test_all_background_frame_every_slot_absent():
    """HandSegNet weights whose foreground logit is far below zero: det is empty, every slot is absent, and the outputs are finite and
    equal to the chain of per-op calls on the fall-back box."""
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth.make_weights(seg_bias=-60.0))
        e.finalize_weights(0)
        fr = synth.make_batch(9, 2, 240, 320)
        o = HO.check_whole_path(e, fr, 3, expect_all_valid=False)
        assert HO.background_frame_scoremap_is_empty(o)
        assert not o['valid'].any() and not o['area'].any() and not o['mask'].any()
        assert np.all(o['center'] == 160.0) and np.all(o['scale'] == F32(256.0) / (F32(100.0) * F32(1.25)))
        assert np.all(o['kp_crop'] >= 0) and np.isfinite(o['kp_hw']).all()
    finally:
        e.close()


def test_half_precision_trunks(synth_weights):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=_lib.DEFAULT_LIB)
    try:
        e.load_weight_dict(synth_weights)
        e.finalize_weights('f16')
        HO.check_whole_path(e, synth.make_batch(0, 2, 240, 320), 4, expect_all_valid=False)
        HO.assert_k1_is_infer_full(e, synth.make_batch(0, 2, 240, 320))
    finally:
        e.close()


def test_errors_are_loud(eng):
    fr = synth.make_batch(0, 1, 240, 320)
    from hand3d_amd import _lib
    hs = HO.hand_sides(1, 4)
    for K in (0, 5):
        assert eng.lib.hp3d_infer_hands(eng.h, 1, 240, 320, K, _lib._ptr(fr), _lib._ptr(hs), *[None] * 11) == -1
        assert "max hands" in eng.lib.hp3d_last_error(eng.h).decode()
    with pytest.raises(AssertionError, match="max hands"):
        eng.masks_from_scoremap(synth.blob_scoremap('one_blob'), 5)
    assert eng.lib.hp3d_infer_hands(eng.h, 1, 240, 320, 2, _lib._ptr(fr), None, *[None] * 11) == -1
    assert "hand_side is NULL" in eng.lib.hp3d_last_error(eng.h).decode()
    eng.set_option('mask_grow', 'lds')
    try:
        with pytest.raises(AssertionError, match="too large for the in-LDS mask growth"):
            eng.infer_hands(np.zeros((1, 540, 960, 3), F32), HO.hand_sides(1, 2), 2)
    finally:
        eng.set_option('mask_grow', 'auto')
