"""Mask growth beyond one workgroup's LDS (glue.hip: mask_pack_kernel + mask_grow_global_kernel), on the CPU interpreter.

Frames whose three bit-packed maps exceed the LDS kernel's 159 KB (600x800, 720x1280) must give exactly what
utils/general.py:247-328 gives: the same mask, centre, crop size, scale and seed, bit for bit.  The score maps are built
so that det and the seed are known: fg > 1/2 on det, < 1/2 elsewhere, and one pixel with the unique largest fg."""
import numpy as np
import pytest

from oracle import general as G


def scoremap_from(det, seed):
    """[H,W] det in {0,1} and a (row, col) seed -> [1,H,W,2] logits with that detmap and that arg-max."""
    H, W = det.shape
    sm = np.zeros((1, H, W, 2), np.float32)
    sm[0, :, :, 1] = np.where(det > 0, 2.0, -2.0)
    sm[0, seed[0], seed[1], 1] = 3.0
    return sm


def oracle_mask(sm):
    mask = G.single_obj_scoremap(sm, early_exit=True)[..., 0]
    center, _, size = G.calc_center_bb(mask[..., None])
    return mask, center, size, G.scale_from_crop_size(size), G.find_max_location(G.fg_and_detmap(sm)[0])


def assert_exact(engine, sm):
    before = engine.counter('mask_grow_global_launches')
    got = engine.mask_from_scoremap(sm)
    assert engine.counter('mask_grow_global_launches') == before + 1
    ref = oracle_mask(sm)
    for name, a, b in zip(('mask', 'center', 'crop_size', 'scale', 'seed'), got, ref):
        assert a.shape == b.shape and np.array_equal(a, b), name
    return got


def blob(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0).astype(np.uint8)


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


@pytest.mark.parametrize("H,W", [(600, 800), (720, 1280)])
def test_compact_blob_off_centre(emu_engine, H, W):
    rng = np.random.default_rng(H)
    det = blob(H, W, H // 4, 3 * W // 4, 70, 55)
    det[rng.random((H, W)) < 0.02] = 0           # holes the growth has to go round
    det[H - 60:H - 20, 30:90] = 1                 # a second component, never reached
    m, c, _, _, seed = assert_exact(emu_engine, scoremap_from(det, (H // 4, 3 * W // 4)))
    assert m.sum() > 10000 and m[0, H - 40, 60] == 0 and seed.tolist() == [[H // 4, 3 * W // 4]]


def test_several_components_only_seeded_grows(emu_engine):
    H, W = 600, 800
    det = np.zeros((H, W), np.uint8)
    for cy, cx in ((100, 100), (100, 400), (300, 700), (500, 200), (480, 520)):
        det |= blob(H, W, cy, cx, 40, 50)
    m = assert_exact(emu_engine, scoremap_from(det, (300, 700)))[0]
    assert m.sum() == blob(H, W, 300, 700, 40, 50).sum()


def test_serpentine_stops_at_pass_cap(emu_engine):
    H, W = 600, 800
    det = serpentine(H, W)
    seed = (0, 0)
    _, passes = G.grow_objectmap(det.astype(np.float32), seed, early_exit=True)
    assert passes == max(H, W) // 10                # the cap binds: no fix-point before it
    m = assert_exact(emu_engine, scoremap_from(det, seed))[0]
    assert 0 < m.sum() < det.sum()


def test_det_all_ones_window_spans_frame(emu_engine):
    H, W = 600, 800
    m = assert_exact(emu_engine, scoremap_from(np.ones((H, W), np.uint8), (250, 333)))[0]
    assert m.all()


@pytest.mark.parametrize("mode", ["inf", "fltmax"])
def test_det_all_zeros_empty_fallbacks(emu_engine, monkeypatch, mode):
    H, W = 600, 800
    sm = np.zeros((1, H, W, 2), np.float32)
    sm[..., 1] = -2.0
    sm[0, 321, 123, 1] = -1.0
    monkeypatch.setattr(G, 'EMPTY_REDUCE', mode)
    emu_engine.set_option('empty_reduce', mode)
    try:
        m, c, s, _, _ = assert_exact(emu_engine, sm)
    finally:
        emu_engine.set_option('empty_reduce', 'inf')
    assert not m.any() and s.tolist() == [[100.0]]
    assert c.tolist() == ([[160.0, 160.0]] if mode == 'inf' else [[0.0, 0.0]])


@pytest.mark.parametrize("seed", [(0, 0), (599, 799), (0, 799)])
def test_seed_in_corner(emu_engine, seed):
    H, W = 600, 800
    det = blob(H, W, seed[0], seed[1], 120, 90)
    assert_exact(emu_engine, scoremap_from(det, seed))


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 40, 64), (2, 37, 53), (1, 16, 16), (3, 33, 200)])
def test_global_kernel_equals_lds_kernel(emu_engine, B, H, W):
    rng = np.random.default_rng(B * H * W)
    small = rng.standard_normal((B, max(H // 8, 2), max(W // 8, 2), 2)).astype(np.float32)
    from oracle import tf_ops as T
    sm = T.resize_bilinear_legacy(small, H, W)
    emu_engine.set_option('mask_grow', 'lds')
    try:
        n0 = emu_engine.counter('mask_grow_global_launches')
        lds = emu_engine.mask_from_scoremap(sm)
        assert emu_engine.counter('mask_grow_global_launches') == n0
        emu_engine.set_option('mask_grow', 'global')
        glob = emu_engine.mask_from_scoremap(sm)
        assert emu_engine.counter('mask_grow_global_launches') == n0 + 1
    finally:
        emu_engine.set_option('mask_grow', 'auto')
    for a, b in zip(lds, glob):
        assert np.array_equal(a, b)
    rm = G.single_obj_scoremap(sm)[..., 0]
    assert np.array_equal(glob[0], rm)


def test_lds_mode_still_refuses_large_frames(emu_engine):
    sm = np.zeros((1, 600, 800, 2), np.float32)
    emu_engine.set_option('mask_grow', 'lds')
    try:
        with pytest.raises(AssertionError, match="map too large"):
            emu_engine.mask_from_scoremap(sm)
        with pytest.raises(AssertionError, match="too large for the in-LDS mask growth"):
            emu_engine.infer_full(np.zeros((1, 600, 800, 3), np.float32), np.array([[1, 0]], np.float32))
    finally:
        emu_engine.set_option('mask_grow', 'auto')


def test_frame_envelope_is_refused_before_any_launch(emu_engine):
    with pytest.raises(AssertionError, match=r"must stay below 2\^31"):
        emu_engine.infer_full(np.zeros((1, 2304, 3648, 3), np.float32), np.array([[1, 0]], np.float32))
