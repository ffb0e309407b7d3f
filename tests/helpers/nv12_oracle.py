"""NV12 frames: the test side's own NumPy restatement of the colour rule of include/hp3d.h (not an import of
hand3d_amd.utils.nv12), surfaces whose padding would spoil every result if it were read, synth frames pushed through a forward
conversion, and the cases tests/test_nv12.py and tests/test_gpu_nv12.py share.  Everything an NV12 entry point returns is compared with
the uint8 entry point on `to_rgb` of the same planes, bit for bit: no tolerance anywhere."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_oracle as TO      # noqa: E402

F32 = np.float32
# option value -> ky, yoff, then (cu, cv) for R, G, B: the table of the issue, typed in again
TABLE = {
    'bt709': (298, 16, ((0, 459), (-55, -136), (541, 0))),
    'bt601': (298, 16, ((0, 409), (-100, -208), (516, 0))),
    'bt709_full': (256, 0, ((0, 403), (-48, -120), (475, 0))),
    'bt601_full': (256, 0, ((0, 359), (-88, -183), (454, 0))),
}
MATRICES = tuple(TABLE)
POISON = 255          # padding bytes; random planes hold 0 ... 250, so a padding byte read as a sample changes that sample
# hand-worked (matrix, (Y, U, V)) -> (R, G, B)
TRIPLES = [('bt601', (81, 90, 240), (255, 0, 0)), ('bt601', (145, 54, 34), (0, 255, 1)), ('bt601', (41, 240, 110), (0, 0, 255)),
           ('bt601', (16, 128, 128), (0, 0, 0)), ('bt601', (235, 128, 128), (255, 255, 255)), ('bt709', (81, 90, 240), (255, 24, 0)),
           ('bt601_full', (81, 90, 240), (238, 14, 14))]


def convert(Y, U, V, matrix):
    """int arrays of equal shape -> uint8 [..., 3].  NumPy's floor division by 256 is the arithmetic shift."""
    ky, yoff, rows = TABLE[matrix]
    C, D, E = np.asarray(Y, np.int32) - yoff, np.asarray(U, np.int32) - 128, np.asarray(V, np.int32) - 128
    out = [np.minimum(np.maximum((ky * C + cu * D + cv * E + 128) // 256, 0), 255) for cu, cv in rows]
    return np.stack(out, axis=-1).astype(np.uint8)


def to_rgb(y, uv, W, matrix):
    """Planes [B,H,pitch] / [B,H/2,pitch] -> [B,H,W,3] uint8: pixel (r, c) takes Y at (r, c), U at (r // 2, c - c % 2), V one byte on."""
    twice = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    return np.stack([convert(y[b, :, :W], twice(uv[b, :, 0:W:2]), twice(uv[b, :, 1:W:2]), matrix) for b in range(y.shape[0])])


def surface(B, H, W, pitch, gap_rows=0, tail_rows=0):
    """One decoder-shaped allocation per batch: frame b = H luma rows, gap_rows unused rows, H / 2 chroma rows, tail_rows unused rows, all
    `pitch` bytes wide and POISON wherever no sample lies.  Returns (y, uv) as views: both have the frame stride pitch * rows."""
    rows = H + gap_rows + H // 2 + tail_rows
    s = np.full((B, rows, pitch), POISON, np.uint8)
    return s[:, :H], s[:, H + gap_rows:H + gap_rows + H // 2]


def random_planes(seed, B, H, W, pitch, gap_rows=0, tail_rows=0):
    rng = np.random.default_rng(seed)
    y, uv = surface(B, H, W, pitch, gap_rows, tail_rows)
    y[:, :, :W] = rng.integers(0, 251, (B, H, W))
    uv[:, :, :W] = rng.integers(0, 251, (B, H // 2, W))
    return y, uv


def from_rgb(rgb, pitch=None, gap_rows=0, tail_rows=0):
    """A forward conversion (BT.709 video range, float64, 2 x 2 chroma mean, round) of uint8 RGB [B,H,W,3] into a poisoned surface:
    planes that look like a picture.  Which forward form is used matters to no test: every comparison starts from the planes."""
    B, H, W, _ = rgb.shape
    y, uv = surface(B, H, W, W if pitch is None else pitch, gap_rows, tail_rows)
    p = rgb.astype(np.float64)
    luma = 0.2126 * p[..., 0] + 0.7152 * p[..., 1] + 0.0722 * p[..., 2]
    cb = ((p[..., 2] - luma) / 1.8556).reshape(B, H // 2, 2, W // 2, 2).mean(axis=(2, 4))
    cr = ((p[..., 0] - luma) / 1.5748).reshape(B, H // 2, 2, W // 2, 2).mean(axis=(2, 4))
    q = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    y[:, :, :W] = q(16 + luma * 219 / 255)
    uv[:, :, 0:W:2] = q(128 + cb * 224 / 255)
    uv[:, :, 1:W:2] = q(128 + cr * 224 / 255)
    return y, uv


def synth_planes(seed, t, B, H, W, **kw):
    """The tracking tests' frame t (tests/helpers/track_oracle.py) as NV12 planes."""
    return from_rgb(TO.to_u8(TO.frames(seed, t, B, H, W)), **kw)


def lattice_values():
    return sorted(set([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255]) | set(range(0, 256, 17)))


def lattice_planes():
    """Every (Y, U, V) of lattice_values()^3 once: chroma pair (i, j) owns a column of 2 x 2 blocks that carries the luma values."""
    v = np.array(lattice_values(), np.uint8)
    n = len(v)
    rows = 2 * ((n + 3) // 4)                    # 4 luma values per chroma block
    H, W = max(16, rows), 2 * n * n
    y, uv = surface(1, H, W, W)
    y[:, :, :W] = 0
    uv[:, :, :W] = 128
    uu, vv = np.meshgrid(v, v, indexing='ij')
    uv[0, :, 0:W:2] = uu.reshape(-1)[None, :]
    uv[0, :, 1:W:2] = vv.reshape(-1)[None, :]
    lum = np.resize(v, (rows // 2) * 4).reshape(rows // 2, 2, 2)          # block k holds values 4k ... 4k + 3 (wrapping round)
    y[0, :rows, :W] = np.tile(lum.reshape(rows // 2, 2, 1, 2), (1, 1, n * n, 1)).reshape(rows, W)
    return y, uv, W


def exhaustive_planes():
    """All 2^24 (Y, U, V): B = 4 frames of 2048 x 2048; chroma block g (row-major over the batch's 4 x 1024 x 1024 blocks) holds pair
    (U, V) = divmod(g // 64, 256) and its four luma pixels 4 (g % 64) + 0 ... 3.  pitch = W: 18 MB."""
    g = np.arange(4 * 1024 * 1024, dtype=np.int64).reshape(4, 1024, 1024)
    uv = np.empty((4, 1024, 2048), np.uint8)
    uv[:, :, 0::2] = (g // 64) // 256
    uv[:, :, 1::2] = (g // 64) % 256
    y = np.empty((4, 2048, 2048), np.uint8)
    k = 4 * (g % 64)
    for dr in range(2):
        for dc in range(2):
            y[:, dr::2, dc::2] = k + 2 * dr + dc
    return y, uv


# ---- crop and downscale cases ---------------------------------------------------------------------------------------------------------
CROP_FRAMES = [(16, 16), (18, 22)]


def crop_pitches(W):
    return [W, W + 2, 64]


def crop_boxes(H, W, B, K, rng, crop):
    """[(center [B K,2], scale [B K])]; a box spans crop / scale pixels.  Inside the frame; half outside each edge; wholly outside; scale
    1 and 10; and windows of 2 and 3 pixels, whose neighbouring taps lie 2 / 7 and 3 / 7 pixels apart: tap pairs (tx0, tx0 + 1) that
    share a chroma block (tx0 even) and pairs that straddle two (tx0 odd) both occur, in rows as in columns."""
    n = B * K
    t = lambda c: np.tile(np.array(c, F32), (n, 1))
    span = lambda px: np.full(n, crop / px, F32)
    out = [(rng.uniform(6, [H - 6, W - 6], (n, 2)).astype(F32), (crop / rng.uniform(2, 12, n)).astype(F32))]
    out += [(t(c), span(8.0)) for c in ([0.0, W / 2], [H - 1.0, W / 2], [H / 2, 0.0], [H / 2, W - 1.0])]
    out += [(t([-3.0 * H, 5.0 * W]), span(4.0))]
    out += [(rng.uniform(0, [H, W], (n, 2)).astype(F32), np.full(n, s, F32)) for s in (1.0, 10.0)]
    out += [(t([H / 2 + 0.25, W / 2 + 0.5]), span(px)) for px in (2.0, 3.0)]
    return out


# (B, H, W, f, pitch): the issue's list; (1, 32, 64, f) at pitch 64 takes the wide path, at 66 the element path
DOWNSCALE_CASES = [(1, 16, 16, 2, 16), (2, 18, 22, 4, 24), (1, 34, 38, 8, 40), (1, 18, 22, 3, 22), (1, 16, 24, 5, 26), (1, 32, 64, 7, 64)]
DOWNSCALE_CASES += [(1, 32, 64, f, p) for f in (2, 4, 8) for p in (64, 66)]
DOWNSCALE_CASES += [(2, 32, 64, 4, 64), (3, 16, 16, 1, 16), (2, 18, 22, 1, 26)]


def assert_crop_cases(e, H, W, pitch, matrix='bt709', crop=8):
    """crop_and_resize_nv12 == crop_and_resize_u8 / crop_and_resize_idx on the converted frame, B = 2 with a frame stride above the
    minimum; K = 1 and 2; the idx form with m < B K."""
    B = 2
    rng = np.random.default_rng(H * 100 + W + pitch)
    y, uv = random_planes(H + pitch, B, H, W, pitch, gap_rows=1, tail_rows=2)
    rgb = to_rgb(y, uv, W, matrix)
    e.set_option('nv12_matrix', matrix)
    try:
        assert np.array_equal(e.nv12_to_rgb(y, uv, W), rgb)
        n0 = e.counter('crop_nv12_launches')
        calls = 0
        for K in (1, 2):
            for center, scale in crop_boxes(H, W, B, K, rng, crop):
                got = e.crop_and_resize_nv12(y, uv, center, scale, W=W, K=K, crop_size=crop)
                if K == 1:
                    want = e.crop_and_resize_u8(rgb, center, scale, crop)
                else:
                    want = e.crop_and_resize_idx(rgb, center, scale, np.arange(B * K), K, crop)
                assert np.array_equal(got, want), (H, W, pitch, K)
                calls += 1
            idx = np.array([B * K - 1, 0, 1][:B * K - 1], np.int32)          # m < B K, not ascending, a slot of each frame
            got = e.crop_and_resize_nv12(y, uv, center, scale, W=W, K=K, idx=idx, crop_size=crop)
            assert np.array_equal(got, e.crop_and_resize_idx(rgb, center, scale, idx, K, crop)), (H, W, pitch, K, 'idx')
            calls += 1
        assert e.counter('crop_nv12_launches') == n0 + calls
        # the interior box's crop is a picture, the outside one's is the extrapolation value
        c, s = crop_boxes(H, W, B, 1, rng, crop)[5]
        assert not e.crop_and_resize_nv12(y, uv, c, s, W=W, crop_size=crop).any()
    finally:
        e.set_option('nv12_matrix', 'bt709')


def assert_downscale_case(e, B, H, W, f, pitch, matrix='bt709'):
    """downscale_nv12 == downscale_u8 (f = 1: preprocess_u8 at equal sizes) on the converted frame; the idx form on a subset."""
    y, uv = random_planes(B * 1000 + H + W + f, B, H, W, pitch, gap_rows=0 if pitch % 8 == 0 else 1, tail_rows=2 if B > 1 else 0)
    rgb = to_rgb(y, uv, W, matrix)
    e.set_option('nv12_matrix', matrix)
    try:
        want = e.preprocess_u8(rgb, H, W) if f == 1 else e.downscale_u8(rgb, f)
        assert np.array_equal(e.downscale_nv12(y, uv, f, W=W), want), (B, H, W, f, pitch)
        idx = np.array([B - 1] if B < 3 else [0, B - 1], np.int32)
        assert np.array_equal(e.downscale_nv12(y, uv, f, W=W, idx=idx), want[idx]), (B, H, W, f, pitch, 'idx')
    finally:
        e.set_option('nv12_matrix', 'bt709')


def assert_equal_outputs(a, b, what=''):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def profile_rows(e, call):
    e.set_profiling(1)
    try:
        o = call()
        rows = [r[0] for r in e.profile()]
    finally:
        e.set_profiling(0)
    return o, rows


def assert_tracked_rows(rows, chunks=1, idx=False):
    """A tracked NV12 step: exactly one NV12 crop row per chunk and no other launch that reads a frame."""
    name = 'crop_and_resize_idx_nv12' if idx else 'crop_and_resize_nv12'
    assert rows.count(name) == chunks, rows
    bad = [r for r in rows if r.startswith(('preprocess', 'downscale')) or (r.startswith('crop_and_resize') and r != name)]
    assert not bad, bad
