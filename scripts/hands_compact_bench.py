"""Option "hands_compact"  against its yardstick: seeded tracked steps of hp3d_track_hands_step_dev with the option off
and on, where only `nvalid` of the K slots of every frame hold a hand, and -- the yardstick -- a seeded tracked step of
hp3d_track_step_dev at batch m = B * nvalid on the same context in the same run: the same back-half launches without gather and
scatter.  float32, device-resident frames, _dev entry points with every output (crop and heat maps included: the scatter's traffic), one
context per cell, warm-up, then the median of three timed regions and their spread, as scripts/track_hands_bench.py does.  Every timed
step has its seed call in front (so that it is a tracked step whatever random-weight keypoints say); the seed calls are timed on their
own and a STEP's time is the seeded figure less the seed's.  One more cell times hp3d_infer_hands_dev on the synthetic frames with
whatever valid count they give (reported), off and on, with the same yardstick at batch m beside it.  The event-timed `slot_scatter` row
comes with the bytes it moved (read + written) and the GB/s.  Writes one JSON line to profiles/hands_compact_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand3d_amd import _lib, synth      # noqa: E402

STEP_OUT = (('crop', 256 * 256 * 3 * 4), ('kpmap', 256 * 256 * 21 * 4), ('coord3d', 63 * 4), ('kp_hw', 42 * 8), ('kp_crop', 42 * 4), ('center', 8),
            ('scale', 4), ('confidence', 4), ('lost', 4), ('detected', 4), ('valid', 4), ('area', 4), ('claimed', 4))
SINGLE_KEYS = ('crop', 'kpmap', 'coord3d', 'kp_hw', 'kp_crop', 'center', 'scale', 'confidence', 'lost', 'detected')
HANDS_KEYS = ('crop', 'kpmap', 'coord3d', 'kp_hw', 'kp_crop', 'center', 'scale', 'valid', 'area')


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


def engine():
    e = _lib.Engine(0)
    e.load_weight_dict(synth.make_weights())
    e.finalize_weights(0)
    return e


def scatter_row(e):
    for name, _, ms, _, nbytes in e.profile():
        if name == 'slot_scatter':
            return {'ms': round(ms, 4), 'bytes': int(nbytes), 'GBps': round(nbytes / ms / 1e6, 1) if ms > 0 else None}
    return None


def tracked_cell(B, K, H, W, nvalid, steps, warmup):
    e = engine()
    n, m = B * K, B * nvalid
    img, hs = synth.make_batch(B, B, H, W), synth.hand_sides(n)
    rng = np.random.default_rng(K)
    c = (rng.uniform(0.3, 0.7, (B, K, 2)) * [H, W]).astype(np.float32)
    s = np.full((B, K), 2.0, np.float32)
    v = np.zeros((B, K), np.int32)
    v[:, :nvalid] = 1
    idx = np.flatnonzero(v.reshape(-1))
    d_img, d_hs = e.to_device(img), e.to_device(hs)
    d_img_m, d_hs_m = e.to_device(img[idx // K]), e.to_device(hs[idx])          # the yardstick's batch: the valid slots' frames
    out = {k: e.dev_alloc(n * b) for k, b in STEP_OUT}
    ptr = lambda keys: {k: int(out[k]) for k in keys}
    seed_h = lambda: e.track_hands_seed(c, s, v, H, W)
    seed_1 = lambda: e.track_seed(c.reshape(n, 2)[idx], s.reshape(n)[idx], H, W)

    def step_h():
        seed_h(); e.track_hands_step_dev(B, H, W, K, d_img, d_hs, **ptr([k for k, _ in STEP_OUT]))

    def step_1():
        seed_1(); e.track_step_dev(m, H, W, d_img_m, d_hs_m, **ptr(SINGLE_KEYS))
    r = {'kind': 'tracked', 'B': B, 'K': K, 'H': H, 'W': W, 'valid_per_frame': nvalid, 'slots': n, 'slots_run': m, 'spread_ms': {}}
    for opt, key in (('0', 'off'), ('1', 'on')):
        e.set_option('hands_compact', opt)
        for _ in range(warmup):
            step_h()
        n0, w0 = e.counter('track_hands_tracked_steps'), e.counter('hands_compact_waits')
        r['seeded_%s_ms' % key], r['spread_ms'][key] = median3(step_h, steps, e.sync)
        assert e.counter('track_hands_tracked_steps') - n0 == 3 * steps, "a timed step was not a tracked one"
        assert e.counter('hands_compact_waits') == w0, "a tracked step waited for flags"
    for _ in range(warmup):
        step_1()
    n0 = e.counter('track_tracked_steps')
    r['seeded_yardstick_ms'], r['spread_ms']['yardstick'] = median3(step_1, steps, e.sync)
    assert e.counter('track_tracked_steps') - n0 == 3 * steps
    r['seed_hands_ms'] = median3(seed_h, steps, e.sync)[0]
    r['seed_single_ms'] = median3(seed_1, steps, e.sync)[0]
    r['off_ms'] = r['seeded_off_ms'] - r['seed_hands_ms']
    r['on_ms'] = r['seeded_on_ms'] - r['seed_hands_ms']
    r['yardstick_ms'] = r['seeded_yardstick_ms'] - r['seed_single_ms']
    r['on_over_yardstick'] = r['on_ms'] / r['yardstick_ms']
    r['off_over_on'] = r['off_ms'] / r['on_ms']
    e.set_profiling(1)
    step_h(); e.sync()
    r['slot_scatter'] = scatter_row(e)
    r['rows_ms'] = {name: round(ms, 4) for name, _, ms, _, _ in e.profile() if name in ('slot_gather', 'crop_and_resize_idx', 'track_hands_box', 'kp_detect', 'kp_upsample')}
    e.set_profiling(0)
    e.close()
    return r


def hands_cell(B, K, H, W, steps, warmup):
    e = engine()
    n = B * K
    img, hs = synth.make_batch(0, B, H, W), synth.hand_sides(n)
    d_img, d_hs = e.to_device(img), e.to_device(hs)
    out = {k: e.dev_alloc(n * b) for k, b in STEP_OUT}
    ptr = lambda keys: {k: int(out[k]) for k in keys}
    hands = lambda: e.infer_hands_dev(B, H, W, K, d_img, d_hs, **ptr(HANDS_KEYS))
    valid = e.infer_hands(img, hs.reshape(B, K, 2), K, outputs=())['valid']
    idx = np.flatnonzero(valid.reshape(-1))
    m = int(idx.size)
    r = {'kind': 'infer_hands', 'B': B, 'K': K, 'H': H, 'W': W, 'valid': valid.tolist(), 'slots': n, 'slots_run': m, 'spread_ms': {}}
    for opt, key in (('0', 'off'), ('1', 'on')):
        e.set_option('hands_compact', opt)
        for _ in range(warmup):
            hands()
        w0 = e.counter('hands_compact_waits')
        r['%s_ms' % key], r['spread_ms'][key] = median3(hands, steps, e.sync)
        r['waits_per_call_%s' % key] = (e.counter('hands_compact_waits') - w0) / (3.0 * steps)
    r['off_over_on'] = r['off_ms'] / r['on_ms']
    if m:          # the yardstick: a seeded tracked step at batch m (the back half of the m hands, without HandSegNet and the wait)
        c = np.tile(np.array([H / 2.0, W / 2.0], np.float32), (m, 1))
        d_img_m, d_hs_m = e.to_device(img[idx // K]), e.to_device(hs[idx])

        def step_1():
            e.track_seed(c, np.full(m, 2.0, np.float32), H, W); e.track_step_dev(m, H, W, d_img_m, d_hs_m, **ptr(SINGLE_KEYS))
        for _ in range(warmup):
            step_1()
        seeded, r['spread_ms']['yardstick'] = median3(step_1, steps, e.sync)
        r['yardstick_ms'] = seeded - median3(lambda: e.track_seed(c, np.full(m, 2.0, np.float32), H, W), steps, e.sync)[0]
    e.set_profiling(1)
    hands(); e.sync()
    r['slot_scatter'] = scatter_row(e)
    e.set_profiling(0)
    e.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hands_compact_bench.json'))
    a = ap.parse_args()
    cells = [tracked_cell(8, 4, 320, 320, nv, a.steps, a.warmup) for nv in (1, 2, 4)]
    cells.append(tracked_cell(1, 4, 1080, 1920, 1, a.steps, a.warmup))
    cells.append(hands_cell(4, 4, 320, 320, a.steps, a.warmup))
    line = json.dumps({'bench': 'hands_compact', 'steps': a.steps, 'warmup': a.warmup, 'cells': cells})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
