"""Several hands per frame against the single-hand path: hp3d_infer_hands_dev at K = 1, 2, 4 and
hp3d_infer_full_kp_dev at B and at B * K images, on the same context and device-resident frames, in one process; warm-up, then the
median of three timed regions, as bench.py does.  Shapes: B = 1 240x320, B = 1 1080x1920, B = 16 320x320.  Beside the wall times the
event-timed `mask_grow_multi` row of each K and the `mask_grow` row of the single-hand call.  Writes one JSON line to
profiles/hands_bench.json."""
import argparse
import json
import os
import sys
import time

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


def row_ms(e, fn, name):
    e.set_profiling(1)
    fn(); e.sync()
    ms = sum(r[2] for r in e.profile() if r[0] == name)
    e.set_profiling(0)
    return round(ms, 4)


def case(e, B, H, W, steps, warmup, ks=(1, 2, 4)):
    kmax = max(ks)
    img = synth.make_batch(B, B * kmax, H, W)          # B * K frames for full_ms(B * K); the first B are the hands calls' frames
    hs = synth.hand_sides(B * kmax)
    d_img, d_hs = e.to_device(img), e.to_device(hs)
    n = B * kmax
    out = {k: e.dev_alloc(v) for k, v in (('coord3d', n * 63 * 4), ('kp_hw', n * 42 * 8), ('kp_crop', n * 42 * 4), ('center', n * 8),
                                          ('scale', n * 4), ('valid', n * 4), ('area', n * 4))}
    single = {k: int(v) for k, v in out.items() if k not in ('valid', 'area')}
    r = {'B': B, 'H': H, 'W': W, 'full_ms': {}, 'hands_ms': {}, 'spread_ms': {}, 'mask_grow_multi_row_ms': {}, 'valid_slots': {}}
    for nb in sorted(set(B * k for k in ks)):
        full = lambda nb=nb: e.infer_full_dev(nb, H, W, d_img, d_hs, **single)
        for _ in range(warmup):
            full()
        r['full_ms'][str(nb)], r['spread_ms']['full_%d' % nb] = median3(full, steps, e.sync)
        if nb == B:
            r['mask_grow_row_ms'] = row_ms(e, full, 'mask_grow')
    for K in ks:
        hands = lambda K=K: e.infer_hands_dev(B, H, W, K, d_img, d_hs, **{k: int(v) for k, v in out.items()})
        for _ in range(warmup):
            hands()
        r['hands_ms'][str(K)], r['spread_ms']['hands_%d' % K] = median3(hands, steps, e.sync)
        r['mask_grow_multi_row_ms'][str(K)] = row_ms(e, hands, 'mask_grow_multi')
        e.sync()
        r['valid_slots'][str(K)] = int(e.to_host(out['valid'], (B * K,), 'int32').sum())
    r['hands_over_full_same_slots'] = {str(K): r['hands_ms'][str(K)] / r['full_ms'][str(B * K)] for K in ks}
    for b in list(out.values()) + [d_img, d_hs]:
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hands_bench.json'))
    a = ap.parse_args()
    e = _lib.Engine(0)
    e.load_weight_dict(synth.make_weights())
    e.finalize_weights(0)
    res = {'bench': 'hands', 'steps': a.steps, 'warmup': a.warmup,
           'cases': [case(e, 1, 240, 320, a.steps, a.warmup), case(e, 1, 1080, 1920, max(a.steps // 2, 5), a.warmup),
                     case(e, 16, 320, 320, max(a.steps // 4, 5), max(a.warmup // 2, 2))]}
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
