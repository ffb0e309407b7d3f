"""A batch of separate surfaces, formats mixed: the test side.  A batch is B surfaces, each an allocation of its own
(an NV12 one: one per plane) with poison wherever no sample lies and its last byte the last used one, so that an over-read shows;
the allocations may be handed out in descending order of addresses, and a record may repeat an earlier surface.  `to_rgb` stacks the
surfaces' RGB frames by the two existing NumPy forms (px_oracle.to_rgb, nv12_oracle.to_rgb); everything a surface entry point
returns is compared with the uint8 entry point on that stack, bit for bit: no tolerance anywhere."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_oracle as NV       # noqa: E402
import px_oracle as PX         # noqa: E402
import track_oracle as TO      # noqa: E402

F32 = np.float32
POISON = PX.POISON
NV12_VALUE = 16          # HP3D_SURF_NV12, typed in again

assert_equal_outputs = NV.assert_equal_outputs
profile_rows = NV.profile_rows
crop_boxes = NV.crop_boxes


def value(fmt):
    """the C ABI's `format`"""
    return NV12_VALUE if fmt == 'nv12' else PX.VALUE[fmt]


def row_bytes(fmt, W):
    return W if fmt == 'nv12' else W * PX.pixel_bytes(fmt)


def _planes(fmt, H):
    """rows of every plane of a surface"""
    return [H, H // 2] if fmt == 'nv12' else [H]


class Batch:
    """surfaces[b]: a view [H,W,pixel_bytes], or a pair of views (y [H,W], uv [H/2,W]); formats[b]: its name; allocs[b]: the
    allocation(s) behind it, one per plane (a repeated surface shares its original's); pitch[b]."""

    def __init__(self):
        self.surfaces, self.formats, self.allocs, self.pitch = [], [], [], []

    def __len__(self):
        return len(self.surfaces)

    def planes(self, b):
        s = self.surfaces[b]
        return list(s) if self.formats[b] == 'nv12' else [s]

    def addresses(self, b):
        return [p.ctypes.data for p in self.planes(b)]


def build(specs, rgb, seed=0, descending=True):
    """specs[b] = (format, dict(pitch=, lead=)) or an int i < b (record b names surface i again); rgb [B,H,W,3] uint8, the pictures
    (a packed surface holds picture b exactly; an NV12 one holds nv12_oracle.from_rgb of it; samples stay below POISON for pictures in
    0 ... 250).  Every plane gets an allocation of its own that starts `lead` bytes past a 64-byte boundary and ends at the plane's last
    used byte; descending: the allocations are handed out from the highest address down, so surface b + 1 lies below surface b."""
    B, H, W, _ = rgb.shape
    assert len(specs) == B
    sizes = []
    for sp in specs:
        if isinstance(sp, int):
            continue
        fmt, kw = sp
        pitch, lead = kw.get('pitch') or row_bytes(fmt, W), kw.get('lead', 0)
        assert pitch >= row_bytes(fmt, W) and (fmt != 'nv12' or (H % 2 == 0 and W % 2 == 0))
        sizes += [lead + pitch * (rows - 1) + row_bytes(fmt, W) for rows in _planes(fmt, H)]
    raw = [np.full(max(sizes) + 64, POISON, np.uint8) for _ in sizes]
    raw.sort(key=lambda a: a.ctypes.data, reverse=descending)
    pool = iter(raw)
    rng = np.random.default_rng(seed)
    out = Batch()
    for b, sp in enumerate(specs):
        if isinstance(sp, int):
            assert sp < b
            for lst in (out.surfaces, out.formats, out.allocs, out.pitch):
                lst.append(lst[sp])
            continue
        fmt, kw = sp
        pitch, lead = kw.get('pitch') or row_bytes(fmt, W), kw.get('lead', 0)
        views, allocs = [], []
        for rows in _planes(fmt, H):
            r = next(pool)
            off = -r.ctypes.data % 64
            n = lead + pitch * (rows - 1) + row_bytes(fmt, W)
            buf = r[off:off + n]
            allocs.append(buf)
            if fmt == 'nv12':
                views.append(np.lib.stride_tricks.as_strided(buf[lead:], (rows, W), (pitch, 1)))
            else:
                pb = PX.pixel_bytes(fmt)
                views.append(np.lib.stride_tricks.as_strided(buf[lead:], (rows, W, pb), (pitch, pb, 1)))
        if fmt == 'nv12':
            y, uv = NV.from_rgb(rgb[b:b + 1])
            views[0][...] = y[0, :, :W]
            views[1][...] = uv[0, :, :W]
            out.surfaces.append((views[0], views[1]))
        else:
            PX.fill(views[0][None], fmt, rgb[b:b + 1], rng)
            out.surfaces.append(views[0])
        out.formats.append(fmt)
        out.allocs.append(allocs)
        out.pitch.append(pitch)
    return out


def random_batch(seed, specs, H, W, **kw):
    """Pictures in 0 ... 250 (never POISON) that depend on (seed, B, H, W) only."""
    return build(specs, np.random.default_rng(seed).integers(0, 251, (len(specs), H, W, 3)).astype(np.uint8), seed=seed + 1, **kw)


def synth_batch(seed, t, specs, H, W, **kw):
    """The tracking tests' frame t (tests/helpers/track_oracle.py), one surface per frame."""
    return build(specs, TO.to_u8(TO.frames(seed, t, len(specs), H, W)), seed=seed + t, **kw)


def to_rgb(batch, matrix='bt709'):
    """The stack rgb[0 .. B) of the definition: uint8 [B,H,W,3]."""
    out = []
    for s, fmt in zip(batch.surfaces, batch.formats):
        if fmt == 'nv12':
            out.append(NV.to_rgb(s[0][None], s[1][None], s[0].shape[1], matrix)[0])
        else:
            out.append(PX.to_rgb(s[None], fmt)[0])
    return np.stack(out)


def assert_poisoned(batch, H, W):
    """Every byte of every allocation that is no sample is POISON, and every allocation ends at its plane's last used byte."""
    for b in range(len(batch)):
        fmt = batch.formats[b]
        for plane, buf in zip(batch.planes(b), batch.allocs[b]):
            rows, rb = plane.shape[0], row_bytes(fmt, W)
            used = np.zeros(buf.size, bool)
            for r in range(rows):
                o = plane[r].ctypes.data - buf.ctypes.data
                used[o:o + rb] = True
            assert used[-1] and np.all(buf[~used] == POISON), (b, fmt)


def records(batch, H, W):
    """[(data address, chroma address or 0, pitch, format name, H, W)] of host surfaces: what Engine.surface_records takes."""
    out = []
    for b in range(len(batch)):
        a = batch.addresses(b)
        out.append((a[0], a[1] if len(a) > 1 else 0, batch.pitch[b], batch.formats[b], H, W))
    return out


def on_device(e, batch, descending=True):
    """Every allocation of the batch (lead bytes, padding and their poison included) into a device allocation of its own, handed out from
    the highest device address down.  Returns (buffers to free, [(data address, chroma address or 0, pitch, format name)])."""
    import ctypes as C
    uniq = {}
    for b in range(len(batch)):
        for buf in batch.allocs[b]:
            uniq.setdefault(buf.ctypes.data, buf)
    size = max(a.size for a in uniq.values())
    bufs = sorted([e.dev_alloc(size) for _ in uniq], key=int, reverse=descending)
    where = {}
    for (addr, a), d in zip(uniq.items(), bufs):
        a = np.ascontiguousarray(a)
        e._chk(e.lib.hp3d_memcpy(e.h, C.c_void_p(int(d)), a.ctypes.data_as(C.c_void_p), a.nbytes, 0))
        where[addr] = int(d)
    recs = []
    for b in range(len(batch)):
        dev = [where[buf.ctypes.data] + (p.ctypes.data - buf.ctypes.data) for p, buf in zip(batch.planes(b), batch.allocs[b])]
        recs.append((dev[0], dev[1] if len(dev) > 1 else 0, batch.pitch[b], batch.formats[b]))
    return bufs, recs


# ---- the shared cases -----------------------------------------------------------------------------------------------------------------
def mixed3(W):
    """B = 3: bgra aligned; bgr at an odd pitch with a 1-byte lead; nv12 at a padded pitch."""
    return [('bgra', dict()), ('bgr', dict(pitch=W * 3 + 1, lead=1)), ('nv12', dict(pitch=W + 10))]


def assert_to_rgb_cases(e, H=16, W=18):
    b = random_batch(7, mixed3(W), H, W)
    assert_poisoned(b, H, W)
    assert np.array_equal(e.surf_to_rgb(b.surfaces, b.formats), to_rgb(b))
    for first in (('abgr', dict(pitch=W * 4 + 4)), ('nv12', dict(pitch=W + 2, lead=1))):
        b = random_batch(8, [first, 0], H, W)          # both records name one surface
        assert b.addresses(0) == b.addresses(1)
        got = e.surf_to_rgb(b.surfaces, b.formats)
        assert np.array_equal(got, to_rgb(b)) and np.array_equal(got[0], got[1])


def packed3(W):
    """mixed3 with a packed surface at a padded pitch where the NV12 one stands: for frames of odd height or width"""
    return mixed3(W)[:2] + [('argb', dict(pitch=W * 4 + 12))]


def assert_crop_cases(e, H, W, crop=8, big=None):
    """crop_and_resize_surf == crop_and_resize_u8 / crop_and_resize_idx on the stack: B = 3 mixed (a frame of odd height or width
    cannot be NV12: there the mixed batch runs on the frame rounded up to even sizes, and a packed-only batch on the frame itself),
    K = 1 and 2, boxes that reach outside the frame (nv12_oracle.crop_boxes), the idx form with slots [5, 0, 2]."""
    Hn, Wn = H + (H & 1), W + (W & 1)
    _crop_batch(e, mixed3(Wn), Hn, Wn, crop, big)
    if (Hn, Wn) != (H, W):
        _crop_batch(e, packed3(W), H, W, crop, None)


def _crop_batch(e, specs, Hn, Wn, crop, big):
    H, W = Hn, Wn
    b = random_batch(H * 100 + W, specs, Hn, Wn)
    rgb = to_rgb(b)
    B = len(b)
    rng = np.random.default_rng(H * 100 + W)
    n0, calls = e.counter('crop_surf_launches'), 0
    outside = None
    for K in (1, 2):
        boxes = crop_boxes(Hn, Wn, B, K, rng, crop)
        for i, (center, scale) in enumerate(boxes):
            for cs in ([crop, big] if big and i == 0 else [crop]):
                got = e.crop_and_resize_surf(b.surfaces, b.formats, center, scale, K=K, crop_size=cs)
                calls += 1
                want = e.crop_and_resize_u8(rgb, center, scale, cs) if K == 1 else e.crop_and_resize_idx(rgb, center, scale, np.arange(B * K), K, cs)
                assert np.array_equal(got, want), (H, W, K, i, cs)
                if K == 1 and i == 0:
                    assert got.any()
                if K == 1 and i == 5:
                    outside = got
        if K == 2:
            idx = np.array([5, 0, 2], np.int32)
            center, scale = boxes[0]
            got = e.crop_and_resize_surf(b.surfaces, b.formats, center, scale, K=K, idx=idx, crop_size=crop)
            calls += 1
            assert np.array_equal(got, e.crop_and_resize_idx(rgb, center, scale, idx, K, crop)), (H, W, 'idx')
    assert outside is not None and not outside.any()          # the extrapolation value outside the frame
    assert e.counter('crop_surf_launches') == n0 + calls


# (name, specs(W), H, W): packed only on 18 x 22, with NV12 on 18 x 24 -- ragged windows at f = 4 and 8.  In 'wide-and-not' surface 0
# qualifies for the wide loads of f = 2, 4 and 8 (base and pitch multiples of 16) and its neighbours do not (a 1-byte lead; an odd pitch).
DOWNSCALE_BATCHES = [
    ('packed', lambda W: [('bgra', dict()), ('bgr', dict(pitch=W * 3 + 1, lead=1)), ('abgr', dict(pitch=W * 4 + 8))], 18, 22),
    ('mixed', mixed3, 18, 24),
    ('wide-and-not', lambda W: [('rgba', dict(pitch=(W * 4 + 15) // 16 * 16)), ('rgba', dict(pitch=(W * 4 + 15) // 16 * 16, lead=1)),
                                ('nv12', dict(pitch=(W + 15) // 16 * 16)), ('nv12', dict(pitch=W + 1)),
                                ('rgb', dict(pitch=(W * 3 + 15) // 16 * 16)), ('rgb', dict(pitch=W * 3 + 1))], 18, 24),
]
DOWNSCALE_FACTORS = [1, 2, 3, 4, 8]


def assert_downscale_case(e, specs, H, W, f, seed=3, idx=(2, 0)):
    """downscale_surf == downscale_u8 (f = 1: preprocess_u8 at equal sizes) on the stack; the idx form with [2, 0]."""
    b = random_batch(seed + H + W, specs, H, W)
    rgb = to_rgb(b)
    want = e.preprocess_u8(rgb, H, W) if f == 1 else e.downscale_u8(rgb, f)
    assert np.array_equal(e.downscale_surf(b.surfaces, b.formats, f), want), (H, W, f)
    idx = np.array(idx, np.int32)
    assert np.array_equal(e.downscale_surf(b.surfaces, b.formats, f, idx=idx), want[idx]), (H, W, f, 'idx')


def assert_tracked_rows(rows, chunks=1, idx=False):
    """A tracked surface step: exactly one surface crop row per chunk and no other launch that reads a frame (no RGB frame is made)."""
    name = 'crop_and_resize_idx_surf' if idx else 'crop_and_resize_surf'
    assert rows.count(name) == chunks, rows
    bad = [r for r in rows if r.startswith(('preprocess', 'downscale', 'surf_to_rgb')) or (r.startswith('crop_and_resize') and r != name)]
    assert not bad, bad


def u8_rows(rows):
    """a surface step's profile rows with _u8 where _surf stands"""
    return [r.replace('_surf', '_u8') for r in rows]
