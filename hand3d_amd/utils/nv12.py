"""NV12 frames on the host: NumPy forms of the engine's colour rule, and a forward conversion for making inputs.

An NV12 frame is a luma plane y [B,H,pitch] and an interleaved chroma plane uv [B,H/2,pitch] (U at even bytes, V at odd ones) of
uint8; the first W bytes of a row are the picture.  `nv12_to_rgb` is the rule of include/hp3d.h bit for bit -- what
Engine.nv12_to_rgb computes on the device.  `rgb_to_nv12` goes the other way to make inputs for tests, examples and benchmarks; it
sits on no parity path: nothing compares the engine with it."""
import numpy as np

# option "nv12_matrix" -> (ky, yoff, (cu, cv) of R, G, B): the rounded coefficients ARE the definition
MATRICES = {
    'bt709': (298, 16, (0, 459), (-55, -136), (541, 0)),
    'bt601': (298, 16, (0, 409), (-100, -208), (516, 0)),
    'bt709_full': (256, 0, (0, 403), (-48, -120), (475, 0)),
    'bt601_full': (256, 0, (0, 359), (-88, -183), (454, 0)),
}
# (Kr, Kb, full range) of the forward conversion
_FORWARD = {'bt709': (0.2126, 0.0722, False), 'bt601': (0.299, 0.114, False), 'bt709_full': (0.2126, 0.0722, True),
            'bt601_full': (0.299, 0.114, True)}


def nv12_to_rgb(y, uv, W=None, matrix='bt709'):
    """y [B,H,pitch], uv [B,H/2,pitch] uint8 -> RGB uint8 [B,H,W,3].  Chroma is replicated over its 2 x 2 block; with int32 C = Y - yoff,
    D = U - 128, E = V - 128 a channel is clamp((ky C + cu D + cv E + 128) >> 8, 0, 255), the shift arithmetic."""
    ky, yoff, *rows = MATRICES[matrix]
    y, uv = np.asarray(y), np.asarray(uv)
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and y.ndim == 3 and uv.ndim == 3
    B, H, pitch = y.shape
    W = pitch if W is None else int(W)
    assert H % 2 == 0 and W % 2 == 0 and W <= pitch and uv.shape == (B, H // 2, pitch)
    c = y[:, :, :W].astype(np.int32) - yoff
    d = np.repeat(np.repeat(uv[:, :, 0:W:2], 2, axis=1), 2, axis=2).astype(np.int32) - 128
    e = np.repeat(np.repeat(uv[:, :, 1:W:2], 2, axis=1), 2, axis=2).astype(np.int32) - 128
    out = np.empty((B, H, W, 3), np.uint8)
    for ch, (cu, cv) in enumerate(rows):
        out[..., ch] = np.clip((ky * c + cu * d + cv * e + 128) >> 8, 0, 255)
    return out


def rgb_to_nv12(rgb, matrix='bt709', pitch=None):
    """RGB uint8 [B,H,W,3] (H, W even) -> (y [B,H,pitch], uv [B,H/2,pitch]): the matrix's forward form in float64, chroma as the mean
    of its 2 x 2 block, rounded to nearest and clipped.  Padding bytes (pitch > W) are zero.  For making inputs only."""
    kr, kb, full = _FORWARD[matrix]
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
    B, H, W, _ = rgb.shape
    assert H % 2 == 0 and W % 2 == 0, "NV12 needs even H and W"
    pitch = W if pitch is None else int(pitch)
    assert pitch >= W
    r, g, b = (rgb[..., i].astype(np.float64) / 255.0 for i in range(3))
    luma = kr * r + (1.0 - kr - kb) * g + kb * b
    pb, pr = 0.5 * (b - luma) / (1.0 - kb), 0.5 * (r - luma) / (1.0 - kr)
    ys, yo, cs = (255.0, 0.0, 255.0) if full else (219.0, 16.0, 224.0)
    mean = lambda p: p.reshape(B, H // 2, 2, W // 2, 2).mean(axis=(2, 4))
    q = lambda v: np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    y = np.zeros((B, H, pitch), np.uint8)
    uv = np.zeros((B, H // 2, pitch), np.uint8)
    y[:, :, :W] = q(yo + ys * luma)
    uv[:, :, 0:W:2] = q(128.0 + cs * mean(pb))
    uv[:, :, 1:W:2] = q(128.0 + cs * mean(pr))
    return y, uv
