"""Tracked steps against the full path: hp3d_infer_full_kp_dev and tracked steps of hp3d_track_step_dev on the same
context and device-resident frames, in one process; warm-up, then the median of three timed regions, as bench.py does.  Also the
B = 1 uint8 host-frame calls at 1080x1920 (hp3d_infer_full_kp_u8 / hp3d_track_step_u8 and the float32 host step).  The yardstick for
a tracked step is the same run's full-path time minus its event-timed HandSegNet stage and soft-max + mask-growth rows: what the
step would cost if skipping were free.  Tracked steps are timed twice: as a video runs them (seeded once, then step after step;
valid only if the counters say that every timed step was a tracked one -- with random weights a step may lose the hand) and with
hp3d_track_seed in front of every step (always tracked; the seed's two uploads and stream synchronise are timed on their own as
well).
Also NV12 frames at B = 1, 1080x1920 against the uint8 and float32 forms of the same run: host-frame tracked
steps, device-frame tracked steps, and the frame-reading rows of a detect step at detect_scale = 4.
Also packed 8-bit frames (BGRA) in the same run: at B = 1, 1080x1920 the host-frame tracked step against the uint8 and
NV12 ones and the device-frame tracked step against the NV12 and float32 ones, and the device-frame step at B = 32, 320x320 (key "px").
Writes one JSON line to profiles/track_bench.json."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand3d_amd import _lib, synth      # noqa: E402


def regions3(fn, steps, sync):
    """ms per call of three timed regions, ascending."""
    ts = []
    for _ in range(3):
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    return sorted(ts)


def median3(fn, steps, sync):
    return regions3(fn, steps, sync)[1]


def spread3(fn, steps, sync):
    """[min, median, max] of three timed regions, ms per call: the spread is what a difference between two medians has to exceed."""
    return [round(t, 4) for t in regions3(fn, steps, sync)]


def case(e, B, H, W, steps, warmup):
    img = synth.make_batch(B, B, H, W)
    hs = synth.hand_sides(B)
    d_img, d_hs = e.to_device(img), e.to_device(hs)
    out = {k: e.dev_alloc(n) for k, n in (('coord3d', B * 63 * 4), ('kp_hw', B * 42 * 8), ('kp_crop', B * 42 * 4), ('center', B * 8),
                                          ('scale', B * 4), ('confidence', B * 4), ('lost', B * 4), ('detected', B * 4))}
    full = lambda: e.infer_full_dev(B, H, W, d_img, d_hs, coord3d=out['coord3d'], kp_crop=out['kp_crop'], kp_hw=out['kp_hw'],
                                    center=out['center'], scale=out['scale'])
    step = lambda: e.track_step_dev(B, H, W, d_img, d_hs, **{k: int(v) for k, v in out.items()})
    # seed with the full path's own boxes: every timed step is a tracked one whatever random-weight keypoints say
    o = e.infer_full(img, hs, outputs=('scale', 'center'))

    seed = lambda: e.track_seed(o['center'], o['scale'], H, W)

    def tracked():
        seed()
        step()
    for _ in range(warmup):
        full(); tracked()
    r = {'B': B, 'H': H, 'W': W}
    r['full_ms'] = median3(full, steps, e.sync)
    n0 = e.counter('track_tracked_steps')
    r['tracked_seeded_ms'] = median3(tracked, steps, e.sync)
    assert e.counter('track_tracked_steps') - n0 == 3 * steps, "a timed step was not a tracked one"
    r['seed_only_ms'] = median3(seed, steps, e.sync)
    # as a video runs it: seeded once, then step after step on the device's own boxes
    seed()
    n0 = e.counter('track_tracked_steps')
    unseeded = median3(step, steps, e.sync)
    r['tracked_unseeded_all_tracked'] = e.counter('track_tracked_steps') - n0 == 3 * steps
    r['tracked_unseeded_ms'] = unseeded if r['tracked_unseeded_all_tracked'] else None
    r['tracked_ms'] = r['tracked_unseeded_ms'] if r['tracked_unseeded_all_tracked'] else r['tracked_seeded_ms']
    e.set_profiling(1)
    full(); e.sync()
    t = e.get_timing()
    glue = sum(ms for name, _, ms, _, _ in e.profile() if name in ('seg_upsample_softmax', 'mask_grow'))
    step_rows = None
    tracked(); e.sync()
    step_rows = {name: round(ms, 4) for name, _, ms, _, _ in e.profile() if not name.startswith(('PoseNet2D/', 'PosePrior', 'ViewpointNet/', 'fc'))}
    tt = e.get_timing()
    e.set_profiling(0)
    r['full_stage_ms'] = {k: round(v, 4) for k, v in t.items()}
    r['tracked_stage_ms'] = {k: round(v, 4) for k, v in tt.items()}
    r['tracked_glue_rows_ms'] = step_rows
    r['softmax_maskgrow_ms'] = round(glue, 4)
    r['yardstick_ms'] = r['full_ms'] - t['HandSegNet'] - glue
    r['tracked_over_yardstick'] = r['tracked_ms'] / r['yardstick_ms']
    r['full_over_tracked'] = r['full_ms'] / r['tracked_ms']
    for b in list(out.values()) + [d_img, d_hs]:
        b.free()
    return r


def host_u8_case(e, H, W, steps, warmup):
    img = synth.make_batch(3, 1, H, W)
    u8 = np.clip(np.rint((img + 0.5) * 255.0), 0, 255).astype(np.uint8)
    hs = synth.hand_sides(1)
    o = e.infer_full(img, hs, outputs=('scale', 'center'))
    kpc, kph, c3 = np.empty((1, 21, 2), np.int32), np.empty((1, 21, 2), np.float64), np.empty((1, 21, 3), np.float32)
    p = _lib._ptr

    def full_u8():
        e._chk(e.lib.hp3d_infer_full_kp_u8(e.h, 1, H, W, p(u8), H, W, p(hs), None, None, None, None, None, p(c3), None, p(kpc), p(kph)))
    lost, det, conf = np.empty(1, np.int32), np.empty(1, np.int32), np.empty(1, np.float32)

    def tracked_u8():
        e.track_seed(o['center'], o['scale'], H, W)
        e._chk(e.lib.hp3d_track_step_u8(e.h, 1, H, W, p(u8), H, W, p(hs), None, None, None, None, p(c3), p(kpc), p(kph), p(conf), p(lost), p(det)))

    def tracked_f32():
        e.track_seed(o['center'], o['scale'], H, W)
        e._chk(e.lib.hp3d_track_step(e.h, 1, H, W, p(img), p(hs), None, None, None, None, p(c3), p(kpc), p(kph), p(conf), p(lost), p(det)))
    for _ in range(warmup):
        full_u8(); tracked_u8(); tracked_f32()
    return {'H': H, 'W': W, 'full_u8_host_ms': median3(full_u8, steps, e.sync), 'tracked_u8_host_ms': median3(tracked_u8, steps, e.sync),
            'tracked_f32_host_ms': median3(tracked_f32, steps, e.sync)}


def nv12_case(e, H, W, steps, warmup):
    """B = 1 at H x W: the NV12 entry points against the uint8 / float32 ones in the same run.  The planes are the synth frame pushed
    through hand3d_amd.utils.nv12.rgb_to_nv12; the uint8 frame is nv12_to_rgb of them, so both sides see the same picture."""
    from hand3d_amd.utils.nv12 import nv12_to_rgb, rgb_to_nv12
    img = synth.make_batch(3, 1, H, W)
    y, uv = rgb_to_nv12(np.clip(np.rint((img + 0.5) * 255.0), 0, 255).astype(np.uint8))
    u8 = nv12_to_rgb(y, uv)
    f32 = (u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    hs = synth.hand_sides(1)
    o = e.infer_full(f32, hs, outputs=('scale', 'center'))
    kpc, kph, c3 = np.empty((1, 21, 2), np.int32), np.empty((1, 21, 2), np.float64), np.empty((1, 21, 3), np.float32)
    lost, det, conf = np.empty(1, np.int32), np.empty(1, np.int32), np.empty(1, np.float32)
    p = _lib._ptr
    seed = lambda: e.track_seed(o['center'], o['scale'], H, W)

    def host_u8():
        seed()
        e._chk(e.lib.hp3d_track_step_u8(e.h, 1, H, W, p(u8), H, W, p(hs), None, None, None, None, p(c3), p(kpc), p(kph), p(conf), p(lost), p(det)))

    def host_nv12():
        seed()
        e._chk(e.lib.hp3d_track_step_nv12(e.h, 1, H, W, p(y), p(uv), W, 0, p(hs), None, None, None, None, p(c3), p(kpc), p(kph), p(conf), p(lost), p(det)))
    surf = np.concatenate([y, uv], axis=1)
    d_f32, d_surf, d_hs = e.to_device(f32), e.to_device(surf), e.to_device(hs)
    out = {k: e.dev_alloc(n) for k, n in (('coord3d', 63 * 4), ('kp_hw', 42 * 8), ('kp_crop', 42 * 4), ('center', 8), ('scale', 4),
                                          ('confidence', 4), ('lost', 4), ('detected', 4))}
    outs = {k: int(v) for k, v in out.items()}

    def dev_f32():
        seed()
        e.track_step_dev(1, H, W, d_f32, d_hs, **outs)

    def dev_nv12():
        seed()
        e.track_step_nv12_dev(1, H, W, int(d_surf), int(d_surf) + H * W, W, 0, d_hs, **outs)
    for _ in range(warmup):
        host_u8(); host_nv12(); dev_f32(); dev_nv12()
    n0 = e.counter('track_tracked_steps')
    r = {'H': H, 'W': W, 'regions': '[min, median, max] ms of three',
         'tracked_u8_host_ms': spread3(host_u8, steps, e.sync), 'tracked_nv12_host_ms': spread3(host_nv12, steps, e.sync),
         'tracked_f32_dev_ms': spread3(dev_f32, steps, e.sync), 'tracked_nv12_dev_ms': spread3(dev_nv12, steps, e.sync)}
    assert e.counter('track_tracked_steps') - n0 == 12 * steps, "a timed step was not a tracked one"
    # the frame-reading rows, event-timed: a tracked step's crop, and a detect step's detection frame + crop at detect_scale = 4.  One
    # pass unrecorded (caches, code objects), then [min, median, max] of three per row
    def rows():
        return {name: ms for name, _, ms, _, _ in e.profile() if name.startswith(('crop_and_resize', 'downscale', 'preprocess'))}

    def rows3(calls):
        got = {k: [] for k in calls}
        for i in range(4):
            for k, fn in calls.items():
                fn()
                e.sync()
                if i:
                    got[k].append(rows())
        return {k: {name: [round(t, 4) for t in sorted(p[name] for p in v)] for name in v[0]} for k, v in got.items()}

    def detect(nv12):
        e.track_reset()
        if nv12:
            e._chk(e.lib.hp3d_track_step_nv12(e.h, 1, H, W, p(y), p(uv), W, 0, p(hs), None, None, None, None, p(c3), p(kpc), p(kph), p(conf), p(lost), p(det)))
        else:
            e._chk(e.lib.hp3d_track_step_u8(e.h, 1, H, W, p(u8), H, W, p(hs), None, None, None, None, p(c3), p(kpc), p(kph), p(conf), p(lost), p(det)))
    e.set_profiling(1)
    r.update(rows3({'tracked_u8_rows_ms': host_u8, 'tracked_nv12_rows_ms': host_nv12, 'tracked_f32_dev_rows_ms': dev_f32,
                    'tracked_nv12_dev_rows_ms': dev_nv12}))
    e.set_option('detect_scale', '4')
    r.update(rows3({'detect_f4_u8_rows_ms': lambda: detect(False), 'detect_f4_nv12_rows_ms': lambda: detect(True)}))
    e.set_profiling(0)
    e.set_option('detect_scale', '1')
    e.track_reset()
    for b in list(out.values()) + [d_f32, d_surf, d_hs]:
        b.free()
    return r


def px_case(e, B, H, W, steps, warmup, host):
    """Tracked steps on packed BGRA frames at pitch 4 W against the NV12, uint8 and float32 forms in the same run: device frames, and
    (host) host frames.  All sides see the same picture: the planes are the synth frames pushed through rgb_to_nv12, the uint8 frame is
    nv12_to_rgb of them, the BGRA surface is from_rgb of that."""
    from hand3d_amd.utils.nv12 import nv12_to_rgb, rgb_to_nv12
    from hand3d_amd.utils.pixels import from_rgb
    img = synth.make_batch(3, B, H, W)
    y, uv = rgb_to_nv12(np.clip(np.rint((img + 0.5) * 255.0), 0, 255).astype(np.uint8))
    u8 = nv12_to_rgb(y, uv)
    bgra = np.ascontiguousarray(from_rgb(u8, 'bgra', fill=255))
    f32 = (u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    hs = synth.hand_sides(B)
    o = e.infer_full(f32, hs, outputs=('scale', 'center'))
    kpc, kph, c3 = np.empty((B, 21, 2), np.int32), np.empty((B, 21, 2), np.float64), np.empty((B, 21, 3), np.float32)
    lost, det, conf = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.float32)
    p = _lib._ptr
    tail = lambda: (p(hs), None, None, None, None, p(c3), p(kpc), p(kph), p(conf), p(lost), p(det))
    seed = lambda: e.track_seed(o['center'], o['scale'], H, W)
    surf = np.concatenate([y, uv], axis=1)
    fs_nv = surf.strides[0]

    def host_u8():
        seed()
        e._chk(e.lib.hp3d_track_step_u8(e.h, B, H, W, p(u8), H, W, *tail()))

    def host_nv12():
        seed()
        e._chk(e.lib.hp3d_track_step_nv12(e.h, B, H, W, p(surf), C.c_void_p(surf.ctypes.data + H * W), W, fs_nv, *tail()))

    def host_px():
        seed()
        e._chk(e.lib.hp3d_track_step_px(e.h, B, H, W, p(bgra), 4 * W, 4 * H * W, 3, *tail()))
    d_f32, d_surf, d_bgra, d_hs = e.to_device(f32), e.to_device(surf), e.to_device(bgra), e.to_device(hs)
    out = {k: e.dev_alloc(B * n) for k, n in (('coord3d', 63 * 4), ('kp_hw', 42 * 8), ('kp_crop', 42 * 4), ('center', 8), ('scale', 4),
                                              ('confidence', 4), ('lost', 4), ('detected', 4))}
    outs = {k: int(v) for k, v in out.items()}

    def dev_f32():
        seed()
        e.track_step_dev(B, H, W, d_f32, d_hs, **outs)

    def dev_nv12():
        seed()
        e.track_step_nv12_dev(B, H, W, int(d_surf), int(d_surf) + H * W, W, fs_nv, d_hs, **outs)

    def dev_px():
        seed()
        e.track_step_px_dev(B, H, W, int(d_bgra), 4 * W, 4 * H * W, 'bgra', d_hs, **outs)
    calls = {'tracked_f32_dev_ms': dev_f32, 'tracked_nv12_dev_ms': dev_nv12, 'tracked_px_dev_ms': dev_px}
    if host:
        calls.update({'tracked_u8_host_ms': host_u8, 'tracked_nv12_host_ms': host_nv12, 'tracked_px_host_ms': host_px})
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    n0 = e.counter('track_tracked_steps')
    r = {'B': B, 'H': H, 'W': W, 'format': 'bgra', 'pitch': 4 * W, 'regions': '[min, median, max] ms of three'}
    r.update({k: spread3(fn, steps, e.sync) for k, fn in calls.items()})
    assert e.counter('track_tracked_steps') - n0 == 3 * steps * len(calls), "a timed step was not a tracked one"
    # the crop row of one tracked step of each device form, event-timed: one pass unrecorded, then [min, median, max] of three
    e.set_profiling(1)
    rows = {}
    for k, fn in (('f32', dev_f32), ('nv12', dev_nv12), ('px', dev_px)):
        ts = []
        for i in range(4):
            fn()
            e.sync()
            if i:
                ts.append(sum(ms for name, _, ms, _, _ in e.profile() if name.startswith('crop_and_resize')))
        rows[k] = [round(t, 4) for t in sorted(ts)]
    e.set_profiling(0)
    r['crop_row_dev_ms'] = rows
    e.track_reset()
    for b in list(out.values()) + [d_f32, d_surf, d_bgra, d_hs]:
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_bench.json'))
    a = ap.parse_args()
    e = _lib.Engine(0)
    e.load_weight_dict(synth.make_weights())
    e.finalize_weights(0)
    res = {'bench': 'track', 'steps': a.steps, 'warmup': a.warmup,
           'cases': [case(e, 1, 240, 320, a.steps, a.warmup), case(e, 1, 1080, 1920, max(a.steps // 2, 5), a.warmup),
                     case(e, 32, 320, 320, max(a.steps // 2, 5), max(a.warmup // 2, 2))],
           'host_u8_1080p': host_u8_case(e, 1080, 1920, max(a.steps // 2, 5), a.warmup),
           'nv12_1080p': nv12_case(e, 1080, 1920, max(a.steps // 2, 5), a.warmup),
           'px': [px_case(e, 1, 1080, 1920, max(a.steps // 2, 5), a.warmup, True),
                  px_case(e, 32, 320, 320, max(a.steps // 2, 5), max(a.warmup // 2, 2), False)]}
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
