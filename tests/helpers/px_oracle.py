"""Packed 8-bit frames: the whole oracle.  `to_rgb` repacks a surface by plain indexing; `surface` makes allocations
whose padding, lead byte and ignored fourth byte would spoil every result if they were read as colour; the cases tests/test_px.py and
tests/test_gpu_px.py share.  Everything a packed entry point returns is compared with the uint8 entry point on `to_rgb` of the same
surface, bit for bit: no tolerance anywhere."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_oracle as NV       # noqa: E402
import track_oracle as TO      # noqa: E402

F32 = np.float32
# format -> (pixel_bytes, byte offsets of R, G, B): the table of include/hp3d.h, typed in again
TABLE = {'rgb': (3, (0, 1, 2)), 'bgr': (3, (2, 1, 0)), 'rgba': (4, (0, 1, 2)), 'bgra': (4, (2, 1, 0)), 'argb': (4, (1, 2, 3)),
         'abgr': (4, (3, 2, 1))}
FORMATS = tuple(TABLE)
VALUE = {f: i for i, f in enumerate(FORMATS)}          # the C ABI's `format`
POISON = 255          # padding bytes; random samples hold 0 ... 250, so a padding byte read as a sample changes that sample

assert_equal_outputs = NV.assert_equal_outputs
profile_rows = NV.profile_rows
crop_boxes = NV.crop_boxes


def pixel_bytes(fmt):
    return TABLE[fmt][0]


def to_rgb(surf, fmt):
    """[B,H,W,pixel_bytes] -> uint8 RGB [B,H,W,3], tight."""
    pb, (r, g, b) = TABLE[fmt]
    assert surf.shape[3] == pb
    out = np.empty(surf.shape[:3] + (3,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = surf[..., r], surf[..., g], surf[..., b]
    return out


def surface(B, H, W, fmt, pitch=None, lead=0, gap_rows=0, tail_rows=0, gap_bytes=0):
    """One allocation for the batch, POISON everywhere: `lead` bytes (0, or 1 for a misaligned base), then frame b at b * frame_stride
    with H rows `pitch` bytes apart; frame_stride = pitch * (H + gap_rows + tail_rows) + gap_bytes (unused rows, and bytes that take
    the stride off every alignment, between the frames).  The allocation ends at the last frame's last used byte, and its first byte
    lies on a 64-byte boundary, so `lead` alone decides the base's alignment.  Returns (view [B,H,W,pixel_bytes], allocation)."""
    pb = pixel_bytes(fmt)
    pitch = W * pb if pitch is None else pitch
    fs = pitch * (H + gap_rows + tail_rows) + gap_bytes
    n = lead + fs * (B - 1) + pitch * (H - 1) + W * pb
    raw = np.full(n + 64, POISON, np.uint8)
    off = -raw.ctypes.data % 64
    buf = raw[off:off + n]
    view = np.lib.stride_tricks.as_strided(buf[lead:], (B, H, W, pb), (fs, pitch, pb, 1))
    return view, buf


def fill(view, fmt, rgb, rng):
    """The colours of `rgb` [B,H,W,3] into the view; the ignored fourth byte gets independent random values."""
    pb, off = TABLE[fmt]
    if pb == 4:
        view[..., 6 - sum(off)] = rng.integers(0, 256, view.shape[:3])          # (the offsets 0 ... 3 add up to 6)
    for c in range(3):
        view[..., off[c]] = rgb[..., c]


def random_surface(seed, B, H, W, fmt, **kw):
    """Samples in 0 ... 250 (never POISON).  The samples depend on (seed, B, H, W) only: surfaces of one seed in different formats,
    pitches and alignments hold the same picture."""
    view, buf = surface(B, H, W, fmt, **kw)
    fill(view, fmt, np.random.default_rng(seed).integers(0, 251, (B, H, W, 3)), np.random.default_rng(seed + 1))
    return view, buf


def relay(rgb, fmt, seed=0, **kw):
    """uint8 RGB frames [B,H,W,3] re-laid as a poisoned surface."""
    B, H, W, _ = rgb.shape
    view, buf = surface(B, H, W, fmt, **kw)
    fill(view, fmt, rgb, np.random.default_rng(seed))
    return view, buf


def synth_surface(seed, t, B, H, W, fmt, **kw):
    """The tracking tests' frame t (tests/helpers/track_oracle.py), re-laid."""
    return relay(TO.to_u8(TO.frames(seed, t, B, H, W)), fmt, seed=seed + t, **kw)


def layout(view):
    """(pitch, frame_stride) of a view."""
    return view.strides[1], view.strides[0]


# ---- crop and downscale cases ---------------------------------------------------------------------------------------------------------
CROP_FRAMES = [(16, 16), (17, 23)]


def crop_pitches(W, pb):
    return [W * pb, W * pb + 1, (W * pb // 64 + 1) * 64]


def assert_crop_cases(e, H, W, fmt, crop=8, big=None):
    """crop_and_resize_px == crop_and_resize_u8 / crop_and_resize_idx on the repacked frame: B = 2 with a frame stride above the
    minimum, every pitch of crop_pitches at lead 0 and 1 (plus one surface whose stride alone is off the 4-byte grid); K = 1 and 2;
    the idx form with m < B K.  All surfaces hold one picture, so the aligned and the misaligned one give equal crops.  big: one
    crop size more for the first surface."""
    B, pb = 2, pixel_bytes(fmt)
    seed = H * 100 + W
    layouts = [dict(pitch=p, lead=l, gap_rows=1, tail_rows=2) for p in crop_pitches(W, pb) for l in (0, 1)]
    layouts.append(dict(pitch=crop_pitches(W, pb)[2], lead=0, gap_rows=1, gap_bytes=2))
    rgb = first = None
    n0, calls = e.counter('crop_px_launches'), 0
    for li, kw in enumerate(layouts):
        s, _ = random_surface(seed, B, H, W, fmt, **kw)
        if rgb is None:
            rgb = to_rgb(s, fmt)
            assert np.array_equal(e.px_to_rgb(s, fmt), rgb)
        assert np.array_equal(to_rgb(s, fmt), rgb)
        rng = np.random.default_rng(seed)
        got_all = []
        for K in (1, 2):
            for center, scale in crop_boxes(H, W, B, K, rng, crop):
                for cs in ([crop, big] if big and li == 0 else [crop]):
                    got = e.crop_and_resize_px(s, fmt, center, scale, K=K, crop_size=cs)
                    calls += 1
                    if li == 0 or cs != crop:
                        want = e.crop_and_resize_u8(rgb, center, scale, cs) if K == 1 else \
                            e.crop_and_resize_idx(rgb, center, scale, np.arange(B * K), K, cs)
                        assert np.array_equal(got, want), (H, W, fmt, kw, K, cs)
                    if cs == crop:
                        got_all.append(got)
            idx = np.array([B * K - 1, 0, 1][:B * K - 1], np.int32)          # m < B K, not ascending, a slot of each frame
            got = e.crop_and_resize_px(s, fmt, center, scale, K=K, idx=idx, crop_size=crop)
            calls += 1
            if li == 0:
                assert np.array_equal(got, e.crop_and_resize_idx(rgb, center, scale, idx, K, crop)), (H, W, fmt, kw, K, 'idx')
            got_all.append(got)
        if first is None:
            first = got_all
            assert any(g.any() for g in first) and not first[5].any()          # pictures, and the extrapolation value outside
        else:          # the other layouts and alignments: the same bits as the first, which equals the uint8 kernels
            for a, b in zip(got_all, first):
                assert np.array_equal(a, b), (H, W, fmt, kw)
    assert e.counter('crop_px_launches') == n0 + calls


# (B, H, W, f, format, pitch kind): the issue's list, the formats cycled; 'tight' = W pb, 'odd' = W pb + 1, '64' = the next multiple of
# 64.  The (1, 32, 64, f) cases run a 3-byte and a 4-byte format, each at a pitch that allows the F-wide path and at an odd one.
DOWNSCALE_CASES = [(1, 16, 16, 2, 'rgb', 'tight'), (2, 18, 22, 4, 'bgr', '64'), (1, 34, 38, 8, 'rgba', '64'), (1, 17, 23, 2, 'bgra', 'tight'),
                   (1, 18, 22, 3, 'argb', 'odd'), (1, 16, 24, 5, 'abgr', 'tight'), (1, 32, 64, 7, 'rgb', 'odd')]
DOWNSCALE_CASES += [(1, 32, 64, f, fmt, p) for f, fmts in ((2, ('bgr', 'bgra')), (4, ('rgb', 'argb')), (8, ('bgr', 'abgr'))) for fmt in fmts
                    for p in ('tight', 'odd')]
DOWNSCALE_CASES += [(2, 32, 64, 4, 'rgba', 'tight'), (2, 32, 64, 4, 'bgr', 'tight'), (3, 16, 16, 1, 'bgra', 'tight'), (2, 17, 23, 1, 'bgr', 'odd'),
                    (2, 17, 23, 1, 'abgr', '64')]


def case_pitch(W, fmt, kind):
    pb = pixel_bytes(fmt)
    return kind if isinstance(kind, int) else dict(zip(('tight', 'odd', '64'), crop_pitches(W, pb)))[kind]


def assert_downscale_case(e, B, H, W, f, fmt, kind):
    """downscale_px == downscale_u8 (f = 1: preprocess_u8 at equal sizes) on the repacked frame; the idx form on a subset."""
    s, _ = random_surface(B * 1000 + H + W + f, B, H, W, fmt, pitch=case_pitch(W, fmt, kind), tail_rows=2 if B > 1 else 0)
    rgb = to_rgb(s, fmt)
    want = e.preprocess_u8(rgb, H, W) if f == 1 else e.downscale_u8(rgb, f)
    assert np.array_equal(e.downscale_px(s, fmt, f), want), (B, H, W, f, fmt, kind)
    idx = np.array([B - 1] if B < 3 else [0, B - 1], np.int32)
    assert np.array_equal(e.downscale_px(s, fmt, f, idx=idx), want[idx]), (B, H, W, f, fmt, kind, 'idx')


def assert_tracked_rows(rows, chunks=1, idx=False):
    """A tracked packed step: exactly one packed crop row per chunk and no other launch that reads a frame."""
    name = 'crop_and_resize_idx_px' if idx else 'crop_and_resize_px'
    assert rows.count(name) == chunks, rows
    bad = [r for r in rows if r.startswith(('preprocess', 'downscale')) or (r.startswith('crop_and_resize') and r != name)]
    assert not bad, bad
