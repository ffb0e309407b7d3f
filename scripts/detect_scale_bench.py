"""Detect steps on a reduced frame: hp3d_track_step_dev with hp3d_track_reset in front of every timed step (so that
each one detects) at detect_scale f = 1, 2 and 4 on device-resident HD frames, one context per cell; warm-up, then the median of three
timed regions and their spread, as bench.py does.  The yardstick of a cell is the same context's hp3d_infer_full_kp_dev at
(B, Hd, Wd) on the detection frame: a detect step at f should cost that call plus the downscale and box rows.  Also per cell: the
event-timed downscale row with its GB/s against the frame bytes read, the box rows, and the context's arena bytes.  f = 1 is the
behaviour without the option.  Sets no gate.  Writes one JSON line to profiles/detect_scale_bench.json."""
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


def cell(weights, B, H, W, f, steps, warmup):
    e = _lib.Engine(0)
    try:
        e.load_weight_dict(weights)
        e.finalize_weights(0)
        e.set_option('detect_scale', str(f))
        img = synth.make_batch(B, B, H, W)
        hs = synth.hand_sides(B)
        d_img, d_hs = e.to_device(img), e.to_device(hs)
        out = {k: e.dev_alloc(n) for k, n in (('coord3d', B * 63 * 4), ('kp_hw', B * 42 * 8), ('kp_crop', B * 42 * 4), ('center', B * 8),
                                              ('scale', B * 4), ('confidence', B * 4), ('lost', B * 4), ('detected', B * 4))}

        def detect():
            e.track_reset()
            e.track_step_dev(B, H, W, d_img, d_hs, **{k: int(v) for k, v in out.items()})
        for _ in range(warmup):
            detect()
        e.sync()
        r = {'B': B, 'H': H, 'W': W, 'f': f, 'arena_bytes': e.counter('arena_bytes')}
        n0 = e.counter('track_detect_steps'), e.counter('detect_scale_steps')
        r['detect_ms'], r['detect_spread_ms'] = median3(detect, steps, e.sync)
        assert e.counter('track_detect_steps') - n0[0] == 3 * steps and e.counter('detect_scale_steps') - n0[1] == (3 * steps if f > 1 else 0)
        e.set_profiling(1)
        detect(); e.sync()
        rows = {name: ms for name, _, ms, _, _ in e.profile()}
        r['stage_ms'] = {k: round(v, 4) for k, v in e.get_timing().items()}
        e.set_profiling(0)
        r['glue_rows_ms'] = {k: round(v, 4) for k, v in rows.items() if not k.startswith(('HandSegNet/', 'PoseNet2D/', 'PosePrior', 'ViewpointNet/', 'fc'))}
        if f > 1:
            r['downscale_ms'] = round(rows['downscale'], 4)
            r['downscale_read_GBps'] = round(B * H * W * 3 * 4 / (rows['downscale'] * 1e-3) / 1e9, 1)
        # the yardstick: the whole path on the detection frame itself, same context
        det = e.downscale(img, f)
        Hd, Wd = det.shape[1:3]
        d_det = e.to_device(det)
        full = lambda: e.infer_full_dev(B, Hd, Wd, d_det, d_hs, coord3d=out['coord3d'], kp_crop=out['kp_crop'], kp_hw=out['kp_hw'],
                                        center=out['center'], scale=out['scale'])
        for _ in range(warmup):
            full()
        r['Hd'], r['Wd'] = Hd, Wd
        r['yardstick_ms'], r['yardstick_spread_ms'] = median3(full, steps, e.sync)
        r['detect_over_yardstick'] = r['detect_ms'] / r['yardstick_ms']
        for b in list(out.values()) + [d_img, d_hs, d_det]:
            b.free()
        return r
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'detect_scale_bench.json'))
    a = ap.parse_args()
    weights = synth.make_weights()
    cells = [cell(weights, B, H, W, f, a.steps, a.warmup) for (B, H, W) in ((1, 720, 1280), (1, 1080, 1920), (4, 1080, 1920)) for f in (1, 2, 4)]
    line = json.dumps({'bench': 'detect_scale', 'steps': a.steps, 'warmup': a.warmup, 'cells': cells})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
