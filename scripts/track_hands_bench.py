"""Tracked steps of the multi-hand tracker against their yardstick: hp3d_track_hands_step_dev at K = 1, 2, 4,
hp3d_infer_hands_dev at the same (B, K) and tracked steps of hp3d_track_step_dev at batch B * K -- the same back-half launches; the box
and crop launches differ -- on the same context and device-resident frames, in one process; warm-up, then the median of three timed
regions (and their spread), as scripts/track_bench.py does.  Tracked steps are timed twice, as there: with the seed call in front of
every step (always a tracked step, whatever random-weight keypoints say; `tracked_*_ms`, the seed calls also on their own), and as a
video runs them -- seeded once, then step after step -- which counts only when the counters say every timed step was a tracked one.
The ratios are formed from a STEP's time (`step_*_ms`): the unseeded figure where it is valid for both trackers, else the seeded figure
less the seed call's own time.  Shapes: B = 1
240x320, B = 1 1080x1920, B = 8 320x320.  Writes one JSON line to profiles/track_hands_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand3d_amd import _lib, synth      # noqa: E402


def median3(fn, steps, sync):
    ts = []
    for _ in range(3):
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    ts.sort()
    return ts[1], ts[2] - ts[0]


def case(e, B, H, W, steps, warmup, ks=(1, 2, 4)):
    kmax = max(ks)
    n = B * kmax
    img = synth.make_batch(B, n, H, W)          # the first B frames are the multi-hand calls'; B * K of them the single-hand tracker's
    hs = synth.hand_sides(n)
    d_img, d_hs = e.to_device(img), e.to_device(hs)
    out = {k: e.dev_alloc(v) for k, v in (('coord3d', n * 63 * 4), ('kp_hw', n * 42 * 8), ('kp_crop', n * 42 * 4), ('center', n * 8),
                                          ('scale', n * 4), ('confidence', n * 4), ('lost', n * 4), ('detected', n * 4), ('valid', n * 4),
                                          ('area', n * 4), ('claimed', n * 4))}
    ptr = lambda keys: {k: int(out[k]) for k in keys}
    single_keys = ('coord3d', 'kp_hw', 'kp_crop', 'center', 'scale', 'confidence', 'lost', 'detected')
    r = {'B': B, 'H': H, 'W': W, 'tracked_hands_ms': {}, 'hands_ms': {}, 'tracked_single_ms': {}, 'seed_hands_ms': {}, 'seed_single_ms': {},
         'spread_ms': {}, 'tracked_over_yardstick': {}, 'hands_over_tracked': {}, 'glue_rows_ms': {}, 'unseeded_all_tracked': {},
         'tracked_hands_unseeded_ms': {}, 'tracked_single_unseeded_ms': {}, 'step_hands_ms': {}, 'step_single_ms': {}}
    for K in ks:
        ns = B * K
        # boxes inside the frame for every slot: seeded, every timed step is a tracked one
        rng = np.random.default_rng(K)
        c = (rng.uniform(0.3, 0.7, (B, K, 2)) * [H, W]).astype(np.float32)
        s = np.full((B, K), 2.0, np.float32)
        v = np.ones((B, K), np.int32)
        seed_h = lambda: e.track_hands_seed(c, s, v, H, W)
        seed_1 = lambda: e.track_seed(c.reshape(ns, 2), s.reshape(ns), H, W)
        step_h = lambda: e.track_hands_step_dev(B, H, W, K, d_img, d_hs, **ptr(out))
        step_1 = lambda: e.track_step_dev(ns, H, W, d_img, d_hs, **ptr(single_keys))
        hands = lambda: e.infer_hands_dev(B, H, W, K, d_img, d_hs, **ptr(('coord3d', 'kp_hw', 'kp_crop', 'center', 'scale', 'valid', 'area')))

        def tracked_h():
            seed_h(); step_h()

        def tracked_1():
            seed_1(); step_1()
        for _ in range(warmup):
            hands(); tracked_h(); tracked_1()
        k = str(K)
        n0 = e.counter('track_hands_tracked_steps')
        r['tracked_hands_ms'][k], r['spread_ms']['tracked_hands_' + k] = median3(tracked_h, steps, e.sync)
        assert e.counter('track_hands_tracked_steps') - n0 == 3 * steps, "a timed step was not a tracked one"
        n0 = e.counter('track_tracked_steps')
        r['tracked_single_ms'][k], r['spread_ms']['tracked_single_' + k] = median3(tracked_1, steps, e.sync)
        assert e.counter('track_tracked_steps') - n0 == 3 * steps, "a timed single-hand step was not a tracked one"
        r['hands_ms'][k], r['spread_ms']['hands_' + k] = median3(hands, steps, e.sync)
        r['seed_hands_ms'][k] = median3(seed_h, steps, e.sync)[0]
        r['seed_single_ms'][k] = median3(seed_1, steps, e.sync)[0]
        # as a video runs it: seeded once, then step after step on the device's own boxes; valid only when the counters say that every
        # timed step was a tracked one (random-weight keypoints may lose a hand)
        seed_h()
        n0 = e.counter('track_hands_tracked_steps')
        t_h, sp_h = median3(step_h, steps, e.sync)
        ok_h = e.counter('track_hands_tracked_steps') - n0 == 3 * steps
        seed_1()
        n0 = e.counter('track_tracked_steps')
        t_1, sp_1 = median3(step_1, steps, e.sync)
        ok_1 = e.counter('track_tracked_steps') - n0 == 3 * steps
        r['unseeded_all_tracked'][k] = bool(ok_h and ok_1)
        r['tracked_hands_unseeded_ms'][k] = t_h if ok_h else None
        r['tracked_single_unseeded_ms'][k] = t_1 if ok_1 else None
        if ok_h and ok_1:
            step_h_ms, step_1_ms = t_h, t_1
            r['spread_ms']['tracked_hands_unseeded_' + k], r['spread_ms']['tracked_single_unseeded_' + k] = sp_h, sp_1
        else:       # the seeded figures less the seed call timed on its own (its uploads and stream synchronise)
            step_h_ms = r['tracked_hands_ms'][k] - r['seed_hands_ms'][k]
            step_1_ms = r['tracked_single_ms'][k] - r['seed_single_ms'][k]
        r['step_hands_ms'][k], r['step_single_ms'][k] = step_h_ms, step_1_ms
        r['tracked_over_yardstick'][k] = step_h_ms / step_1_ms
        r['hands_over_tracked'][k] = r['hands_ms'][k] / step_h_ms
        e.set_profiling(1)
        tracked_h(); e.sync()
        r['glue_rows_ms'][k] = {name: round(ms, 4) for name, _, ms, _, _ in e.profile() if name in ('crop_and_resize', 'kp_detect', 'track_hands_box')}
        e.set_profiling(0)
    e.track_reset()
    e.track_hands_reset()
    for b in list(out.values()) + [d_img, d_hs]:
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_hands_bench.json'))
    a = ap.parse_args()
    e = _lib.Engine(0)
    e.load_weight_dict(synth.make_weights())
    e.finalize_weights(0)
    res = {'bench': 'track_hands', 'steps': a.steps, 'warmup': a.warmup,
           'cases': [case(e, 1, 240, 320, a.steps, a.warmup), case(e, 1, 1080, 1920, max(a.steps // 2, 5), a.warmup),
                     case(e, 8, 320, 320, max(a.steps // 4, 5), max(a.warmup // 2, 2))]}
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
