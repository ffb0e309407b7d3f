"""A batch of separate surfaces against the one-allocation batch: tracked steps at 1080x1920 on device frames, B = 8
and B = 32, in one process; warm-up, then [min, median, max] of three timed regions, as scripts/track_bench.py does.
  a  hp3d_track_step_px_dev on B BGRA frames in ONE allocation: the baseline
  b  hp3d_track_step_surf_dev on the same B frames as B separate allocations: what the table costs
  c  (b) with the formats alternating bgra / nv12: the price of a mixed batch
  d  B calls of hp3d_track_step_px_dev at batch 1: what a multi-stream caller had to do before
Every timed step has hp3d_track_seed in front of it (the frame's centre, scale 1), so it is a tracked step whatever random-weight
keypoints say; (d) seeds each of its B calls, as a caller that keeps one context for B streams must.  The seed alone is timed too
(its uploads and stream synchronise), at batch B and at batch 1.  The crop row of one step of (a), (b) and (c) is event-timed.
Writes one JSON line to profiles/surf_bench.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hand3d_amd import _lib, synth      # noqa: E402
from track_bench import spread3          # noqa: E402


def case(e, B, H, W, steps, warmup):
    from hand3d_amd.utils.nv12 import rgb_to_nv12
    rng = np.random.default_rng(B)
    bgra = rng.integers(0, 256, (B, H, W, 4), dtype=np.uint8)
    hs = synth.hand_sides(B)
    d_all, d_hs = e.to_device(bgra), e.to_device(hs)
    d_each = [e.to_device(bgra[b]) for b in range(B)]
    d_nv = []
    for b in range(1, B, 2):          # the odd frames as NV12: y and uv in one allocation at pitch W
        y, uv = rgb_to_nv12(np.ascontiguousarray(bgra[b:b + 1, :, :, 2::-1]))
        d_nv.append(e.to_device(np.concatenate([y[0], uv[0]], axis=0)))
    same = [(int(d), 0, 4 * W, 'bgra') for d in d_each]
    mixed = [same[b] if b % 2 == 0 else (int(d_nv[b // 2]), int(d_nv[b // 2]) + H * W, W, 'nv12') for b in range(B)]
    out = {k: e.dev_alloc(B * n) for k, n in (('coord3d', 63 * 4), ('kp_hw', 42 * 8), ('kp_crop', 42 * 4), ('center', 8), ('scale', 4),
                                              ('confidence', 4), ('lost', 4), ('detected', 4))}
    outs = {k: int(v) for k, v in out.items()}
    c, s = np.tile(np.array([H / 2.0, W / 2.0], np.float32), (B, 1)), np.ones(B, np.float32)
    seed = lambda: e.track_seed(c, s, H, W)
    seed1 = lambda: e.track_seed(c[:1], s[:1], H, W)

    def a():
        seed()
        e.track_step_px_dev(B, H, W, int(d_all), 4 * W, 4 * H * W, 'bgra', d_hs, **outs)

    def b_():
        seed()
        e.track_step_surf_dev(B, H, W, same, d_hs, **outs)

    def c_():
        seed()
        e.track_step_surf_dev(B, H, W, mixed, d_hs, **outs)

    def d():
        for b in range(B):
            seed1()
            e.track_step_px_dev(1, H, W, int(d_each[b]), 4 * W, 0, 'bgra', d_hs, **outs)

    calls = {'a_px_dev_one_allocation_ms': a, 'b_surf_dev_separate_ms': b_, 'c_surf_dev_bgra_nv12_ms': c_, 'd_px_dev_batch1_x_B_ms': d}
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    n0 = e.counter('track_tracked_steps')
    r = {'B': B, 'H': H, 'W': W, 'regions': '[min, median, max] ms of three'}
    r.update({k: spread3(fn, steps, e.sync) for k, fn in calls.items()})
    assert e.counter('track_tracked_steps') - n0 == 3 * steps * (3 + B), "a timed step was not a tracked one"
    r['seed_batch_B_ms'] = spread3(seed, steps, e.sync)
    r['seed_batch_1_ms'] = spread3(seed1, steps, e.sync)
    # the crop row of one tracked step of (a), (b), (c), event-timed: one pass unrecorded, then [min, median, max] of three
    e.set_profiling(1)
    rows = {}
    for k, fn in (('a', a), ('b', b_), ('c', c_)):
        ts = []
        for i in range(4):
            fn()
            e.sync()
            if i:
                ts.append(sum(ms for name, _, ms, _, _ in e.profile() if name.startswith('crop_and_resize')))
        rows[k] = [round(t, 4) for t in sorted(ts)]
    e.set_profiling(0)
    r['crop_row_ms'] = rows
    e.track_reset()
    for buf in list(out.values()) + [d_all, d_hs] + d_each + d_nv:
        buf.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'surf_bench.json'))
    a = ap.parse_args()
    e = _lib.Engine(0)
    e.load_weight_dict({k: v for k, v in synth.make_weights().items() if not k.startswith('HandSegNet')})
    e.finalize_weights(0)
    res = {'bench': 'surf', 'steps': a.steps, 'warmup': a.warmup, 'cases': [case(e, B, 1080, 1920, a.steps, a.warmup) for B in (8, 32)]}
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
