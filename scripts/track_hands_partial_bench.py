"""Option "track_hands_partial_detect"  against its yardstick, on one GPU with synthetic weights, K = 2 slots per
frame.  A sample is the detect step of a triple (hp3d_track_hands_seed with slot 0 of m frames far outside the frame, a tracked step
that loses exactly those m slots, the detect step behind it), timed by itself with a stream synchronise on each side; a cell's figure is
the median of three regions of `steps` samples.  Every shape is measured with the option off and on in the same process; beside them the
same run's tracked step (seeded, nothing lost, timed the same way) and the HandSegNet + soft-max + multi-hand growth rows of
hp3d_infer_hands on m of the frames (event-timed).  The yardstick of a partial step is tracked step + those rows.
B = 32 at 320 x 320: float32 device-resident frames through hp3d_track_hands_step_dev with every output.  B = 8 at 1080 x 1920: uint8
frames through hp3d_track_hands_step_u8 (the 50 MB upload and the outputs' way back are part of every figure of the cell, the tracked
step's included; no heat maps).  The frames that lose a hand are spread evenly over the batch.  Writes one JSON line to
profiles/track_hands_partial_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand3d_amd import _lib, synth      # noqa: E402

K = 2
FAR = (-5000.0, -7000.0)
OPTION = 'track_hands_partial_detect'
SEG_ROWS = ('seg_upsample_softmax', 'mask_grow_multi')
STEP_ROWS = ('seg_upsample_softmax', 'mask_grow_multi', 'track_hands_partial_index', 'track_hands_slot_gather', 'frame_gather', 'preprocess_u8',
             'preprocess_u8_idx', 'track_hands_select', 'track_hands_select_pos', 'crop_and_resize', 'crop_and_resize_u8')


def median3(sample, steps):
    """sample() returns the milliseconds of one timed step; the median of three regions' means."""
    ts = sorted(sum(sample() for _ in range(steps)) / steps for _ in range(3))
    return ts[1], ts[2] - ts[0]


def lost_set(B, m):
    return [i * B // m for i in range(m)]


def cell(B, H, W, u8, ms_list, steps, warmup):
    e = _lib.Engine(0)
    e.load_weight_dict(synth.make_weights())
    e.finalize_weights(0)
    hs = np.tile(synth.hand_sides(B)[:, None, :], (1, K, 1)).astype(np.float32)
    f0, f1 = synth.make_batch(1, B, H, W), synth.make_batch(2, B, H, W)
    if u8:
        to_u8 = lambda x: np.clip(np.rint((x + 0.5) * 255.0), 0, 255).astype(np.uint8)
        g0, g1 = to_u8(f0), to_u8(f1)
        f1 = (g1.astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
        step = lambda g: e.track_hands_step_u8(g, hs, K)
        lost_of = lambda o: o['lost']
    else:
        d0, d1, d_hs = e.to_device(f0), e.to_device(f1), e.to_device(hs)
        shapes = e._track_hands_outputs(B, K, True)
        out = {k: e.dev_alloc(v.nbytes) for k, v in shapes.items()}
        ptr = {k: int(v) for k, v in out.items()}
        g0, g1 = d0, d1

        def step(g):
            e.track_hands_step_dev(B, H, W, K, g, d_hs, **ptr)
            e.sync()
        lost_of = lambda o: e.to_host(out['lost'], (B, K), np.int32)

    def seed(lost):
        c = np.tile(np.array([H / 2.0, W / 2.0], np.float32), (B, K, 1))
        s = np.full((B, K), 5.0, np.float32)          # a 51.2-pixel crop at the frame's centre: no keypoint can leave the frame
        for b in lost:
            c[b, 0], s[b, 0] = FAR, 1.0
        e.track_hands_seed(c, s, np.ones((B, K), np.int32), H, W)

    def timed(g):
        e.sync()
        t0 = time.perf_counter()
        o = step(g)
        e.sync()
        return (time.perf_counter() - t0) * 1e3, o

    def detect_sample(lost):
        seed(lost)
        got = lost_of(step(g0))          # the tracked step's flags, read before the detect step overwrites the buffer
        return timed(g1)[0], got

    def tracked_sample():
        seed([])
        return timed(g0)[0]

    r = {'B': B, 'K': K, 'H': H, 'W': W, 'cells': [],
         'frames': 'uint8 host (hp3d_track_hands_step_u8)' if u8 else 'float32 device (hp3d_track_hands_step_dev)'}
    for _ in range(warmup):
        tracked_sample()
    n0 = e.counter('track_hands_tracked_steps')
    r['tracked_ms'], r['tracked_spread_ms'] = median3(tracked_sample, steps)
    assert e.counter('track_hands_tracked_steps') - n0 == 3 * steps, "a timed tracked step detected"
    for m in ms_list:
        lost = lost_set(B, m)
        pat = np.zeros((B, K), np.int32)
        pat[lost, 0] = 1
        c = {'m': m, 'lost_frames': lost}
        for opt, key in (('0', 'off'), ('1', 'on')):
            e.set_option(OPTION, opt)
            for _ in range(warmup):
                _, got = detect_sample(lost)
                assert np.array_equal(got, pat), (got, pat)
            n0, p0 = e.counter('track_hands_detect_steps'), e.counter('track_hands_partial_frames_run')
            c['%s_ms' % key], c['%s_spread_ms' % key] = median3(lambda: detect_sample(lost)[0], steps)
            assert e.counter('track_hands_detect_steps') - n0 == 3 * steps, "a timed step was not a detect step"
            c['%s_frames_run_per_step' % key] = (e.counter('track_hands_partial_frames_run') - p0) / (3.0 * steps)
            e.set_profiling(1)          # the rows of one such step (event-timed: serialised, with the profiler's own overhead)
            detect_sample(lost)
            rows = e.profile()
            e.set_profiling(0)
            c['%s_rows_ms' % key] = {
                'HandSegNet': round(sum(t for n, _, t, _, _ in rows if n.startswith('HandSegNet/')), 4),
                **{n: round(sum(t for n2, _, t, _, _ in rows if n2 == n), 4) for n in STEP_ROWS if any(n2 == n for n2, _, _, _, _ in rows)}}
        e.set_option(OPTION, '0')
        e.track_hands_reset()
        e.set_profiling(1)          # hp3d_infer_hands' detection rows at batch m
        e.infer_hands(f1[lost], hs[lost], K, outputs=('scale', 'center'))
        rows = e.profile()
        e.set_profiling(0)
        c['infer_hands_seg_rows_ms'] = round(sum(t for n, _, t, _, _ in rows if n.startswith('HandSegNet/') or n in SEG_ROWS), 4)
        c['yardstick_ms'] = r['tracked_ms'] + c['infer_hands_seg_rows_ms']
        c['on_over_yardstick'] = round(c['on_ms'] / c['yardstick_ms'], 4)
        c['on_over_off'] = round(c['on_ms'] / c['off_ms'], 4)
        r['cells'].append(c)
        print(json.dumps(c), flush=True)
    e.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_hands_partial_bench.json'))
    a = ap.parse_args()
    shapes = [cell(32, 320, 320, False, (1, 4, 16, 32), a.steps, a.warmup), cell(8, 1080, 1920, True, (1, 4, 8), a.steps, a.warmup)]
    line = json.dumps({'bench': 'track_hands_partial', 'steps': a.steps, 'warmup': a.warmup, 'shapes': shapes})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
