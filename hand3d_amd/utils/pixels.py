"""Packed 8-bit frames on the host: NumPy forms of the layouts of include/hp3d.h "packed 8-bit frames".

A packed frame is uint8 [B,H,W,pixel_bytes]; rows may be `pitch` bytes apart (a view).  `to_rgb` is what Engine.px_to_rgb computes on
the device; `from_rgb` lays RGB frames out in a format and at a pitch, for examples, documents and benchmarks."""
import numpy as np

# pixel_format -> (the `format` value of the C ABI, pixel_bytes, byte offsets of R, G, B); the fourth byte is never interpreted
FORMATS = {
    'rgb': (0, 3, (0, 1, 2)),
    'bgr': (1, 3, (2, 1, 0)),
    'rgba': (2, 4, (0, 1, 2)),
    'bgra': (3, 4, (2, 1, 0)),
    'argb': (4, 4, (1, 2, 3)),
    'abgr': (5, 4, (3, 2, 1)),
}
SURF_NV12 = 16          # HP3D_SURF_NV12: the `format` of an NV12 surface in a batch of separate surfaces


def to_rgb(frames, pixel_format):
    """uint8 [B,H,W,pixel_bytes] in `pixel_format` -> RGB uint8 [B,H,W,3] (a copy)."""
    _, pb, off = FORMATS[pixel_format]
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == pb, "frames must be uint8 [B,H,W,%d]" % pb
    return np.ascontiguousarray(frames[..., list(off)])


def from_rgb(rgb, pixel_format, pitch=None, fill=0):
    """RGB uint8 [B,H,W,3] -> uint8 [B,H,W,pixel_bytes] in `pixel_format`, rows `pitch` bytes apart (default: tight).  The result is a
    view into a [B,H,pitch] surface; the fourth byte and the row padding hold `fill`."""
    _, pb, off = FORMATS[pixel_format]
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3, "rgb must be uint8 [B,H,W,3]"
    B, H, W, _ = rgb.shape
    pitch = W * pb if pitch is None else int(pitch)
    assert pitch >= W * pb, "pitch must be at least W * pixel_bytes"
    surf = np.full((B, H, pitch), fill, np.uint8)
    out = surf[:, :, :W * pb].reshape(B, H, W, pb) if pitch == W * pb else np.lib.stride_tricks.as_strided(
        surf, (B, H, W, pb), (H * pitch, pitch, pb, 1))
    for c in range(3):
        out[..., off[c]] = rgb[..., c]
    return out


def surfaces_to_rgb(surfaces, formats, nv12_matrix='bt709'):
    """B separate surfaces -> the stack of their RGB frames, uint8 [B,H,W,3]: a packed surface uint8
    [H,W,pixel_bytes] by `to_rgb`, an NV12 one -- a pair (y [H,W], uv [H/2,W]) under the name 'nv12' -- by utils.nv12.nv12_to_rgb."""
    from .nv12 import nv12_to_rgb
    assert len(surfaces) == len(formats) and len(surfaces) > 0, "one format per surface"
    out = []
    for s, f in zip(surfaces, formats):
        if f == 'nv12':
            out.append(nv12_to_rgb(np.asarray(s[0])[None], np.asarray(s[1])[None], matrix=nv12_matrix)[0])
        else:
            out.append(to_rgb(np.asarray(s)[None], f)[0])
    return np.stack(out)
