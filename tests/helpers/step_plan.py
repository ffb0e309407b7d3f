"""The plan of a tracking / multi-hand call as data: for each scenario below the ordered profile row names, the deltas of every launch
counter and a SHA-1 of every output array, per step.  tests/golden/step_plan.json holds what the library of the commit BEFORE the step
functions were rebuilt from shared helpers gave (one section from the CPU interpreter, one from the GPU: kernel choice differs between
the two); tests/test_step_plan.py and tests/test_gpu_step_plan.py demand equality with it, so a change to the host code of
hp3d_track_step*, hp3d_track_hands_step* or hp3d_infer_hands* that moves, adds or drops a launch, or changes a byte of an output, fails.

As a script it records such a section with any library:
    python tests/helpers/step_plan.py --lib PATH --out FILE [--jobs N] [--names a,b,...]
(--jobs: that many processes, each with an engine of its own on a share of the scenarios; the interpreter needs about a minute per
slot and step.)"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from hand3d_amd import synth                      # noqa: E402
from hand3d_amd.utils import nv12 as NV           # noqa: E402
import track_oracle as TO                         # noqa: E402

F32 = np.float32
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'step_plan.json')

# every counter of hp3d_get_counter's table (the gauges "arena_bytes", "comm_ranks" and the interpreter's "emu_soff_overreads" are sizes
# and diagnostics, not launch counts)
COUNTERS = ('graph_captures', 'graph_replays', 'lift_overlap_calls', 'mask_grow_global_launches', 'mask_grow_multi_launches',
            'conv_h16_launches', 'conv_h16_first_resident_launches', 'first_touch_launches', 'conv_first_launches', 'lift_fused_launches',
            'conv_wino4_tail_launches', 'conv_pw2_launches', 'conv_wino7_split_launches', 'conv_wino7_launches', 'fc_tail_launches',
            'conv_s2_gemm_launches', 'conv_wino4s_launches', 'conv_wino4s_tail_launches', 'conv_wino4_launches', 'conv_wino2_launches',
            'conv_wino_launches', 'conv_mfma_launches', 'conv_splitk_reduce_launches', 'track_detect_steps', 'track_tracked_steps',
            'track_hands_detect_steps', 'track_hands_tracked_steps', 'crop_u8_launches', 'detect_scale_steps', 'hands_compact_slots_run',
            'hands_compact_slots_skipped', 'hands_compact_waits', 'track_partial_frames_run', 'track_partial_frames_skipped',
            'frame_gather_launches', 'crop_nv12_launches')
OPTION_DEFAULTS = {'track_redetect': '0', 'detect_scale': '1', 'hands_compact': '0', 'track_partial_detect': '0', 'micro_batch': 'auto'}
FAR = (-5000.0, -7000.0)          # a seed centre far outside the frame: the tracked step behind it reports the hand as lost


def _scenarios():
    """name -> dict(api, frame, B, H, W, K, opts, seed, steps, prof, kpmap).  api: 'track' | 'hands' | 'infer'; frame: 'f32' (host),
    'dev' (float32 on the device), 'u8', 'nv12' (host); seed: None (a reset: the first step is a fresh detect step), for 'track' a list
    of frames seeded FAR (the others at the frame's centre with scale 10, where nothing is lost: test_track.py), for 'hands' the valid
    flags [B][K]; prof: the profiling mode."""
    S = {}

    def add(name, api, frame, B=1, H=32, W=32, K=1, opts=None, seed=None, steps=1, prof=1, kpmap=True):
        S[name] = dict(api=api, frame=frame, B=B, H=H, W=W, K=K, opts=dict(opts or {}), seed=seed, steps=steps, prof=prof, kpmap=kpmap)

    # the single-hand tracker: frame type x step type
    for fr in ('f32', 'dev', 'u8', 'nv12'):
        add('track_%s_fresh' % fr, 'track', fr)
        add('track_%s_tracked' % fr, 'track', fr, seed=[])
        add('track_%s_lost_then_detect' % fr, 'track', fr, seed=[0], steps=2)
        add('track_%s_scheduled' % fr, 'track', fr, seed=[], opts={'track_redetect': '1'}, kpmap=False)
    for fr in ('f32', 'u8'):
        add('track_%s_detect_scale2' % fr, 'track', fr, H=64, W=64, opts={'detect_scale': '2'})
    # track_partial_detect, B = 3, frame 1 lost: one partial chunk | at micro_batch = 2 a partial chunk (m = 1 of 2) and one with m = 0
    add('track_partial', 'track', 'f32', B=3, seed=[1], steps=2, opts={'track_partial_detect': '1'})
    add('track_partial_two_chunks', 'track', 'f32', B=3, seed=[1], steps=2, opts={'track_partial_detect': '1', 'micro_batch': '2'})
    # profiling: mode 2 accumulates over two steps | mode 1 and two chunks are one profile
    add('track_profiling2', 'track', 'f32', seed=[], steps=2, prof=2)
    add('track_two_chunks', 'track', 'f32', B=2, seed=[], opts={'micro_batch': '1'})
    # the multi-hand tracker, K = 2
    hands = dict(H=48, W=64, K=2)
    add('hands_fresh', 'hands', 'f32', **hands)
    add('hands_tracked_absent', 'hands', 'f32', seed=[[1, 0]], **hands)
    add('hands_tracked_absent_compact', 'hands', 'f32', seed=[[1, 0]], opts={'hands_compact': '1'}, **hands)
    add('hands_fresh_compact', 'hands', 'f32', opts={'hands_compact': '1'}, **hands)
    add('hands_nv12_tracked_compact', 'hands', 'nv12', seed=[[1, 0]], opts={'hands_compact': '1'}, **hands)
    add('hands_two_chunks_compact', 'hands', 'f32', B=2, seed=[[1, 0], [1, 1]], opts={'hands_compact': '1', 'micro_batch': '2'}, **hands)
    # ... a scheduled detect step keeps the seeded slots (the claim rule); on uint8 frames with the option the crop comes from the
    # normalised frame on the detect step and from the frame itself on the tracked one
    add('hands_scheduled', 'hands', 'f32', seed=[[1, 0]], opts={'track_redetect': '1'}, kpmap=False, **hands)
    add('hands_u8_scheduled_compact', 'hands', 'u8', seed=[[1, 0]], opts={'track_redetect': '1', 'hands_compact': '1'}, **hands)
    add('hands_u8_tracked_compact', 'hands', 'u8', seed=[[0, 1]], opts={'hands_compact': '1'}, **hands)
    add('hands_dev_tracked', 'hands', 'dev', seed=[[1, 1]], **hands)
    add('hands_detect_scale2', 'hands', 'f32', H=64, W=64, K=2, opts={'detect_scale': '2'})
    # hp3d_infer_hands*
    for fr in ('f32', 'dev'):
        add('infer_hands_%s' % fr, 'infer', fr, **hands)
        add('infer_hands_%s_compact' % fr, 'infer', fr, opts={'hands_compact': '1'}, **hands)
    return S


SCENARIOS = _scenarios()
CHEAPEST = ('track_f32_tracked', 'track_u8_tracked')          # one tracked step at B = 1: no HandSegNet pass


def _digest(a):
    return 'none' if a is None else hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _on_device(e, call, o, *inputs):
    """A device-pointer call: the inputs uploaded, every output of `o` that is not None in a device buffer, fetched behind a sync."""
    ins = [e.to_device(a) for a in inputs]
    bufs = {k: e.dev_alloc(v.nbytes) for k, v in o.items() if v is not None}
    call(*ins, **bufs)
    e.sync()
    out = {k: (None if v is None else e.to_host(bufs[k], v.shape, v.dtype)) for k, v in o.items()}
    for b in ins + list(bufs.values()):
        b.free()
    return out


def _step(e, sc, t):
    B, H, W, K = sc['B'], sc['H'], sc['W'], sc['K']
    fr = TO.frames(31, t, B, H, W)
    api, kind, kp = sc['api'], sc['frame'], sc['kpmap']
    hs = synth.hand_sides(B * K).reshape((B, 2) if api == 'track' else (B, K, 2))
    if api == 'infer':
        if kind == 'f32':
            return e.infer_hands(fr, hs, K, want_mask=True, outputs=e._HANDS_ORDER)
        o = e._hands_outputs(B, K, H, W, True, e._HANDS_ORDER)
        return _on_device(e, lambda i, h, **kw: e.infer_hands_dev(B, H, W, K, i, h, **kw), o, fr, hs)
    k = () if api == 'track' else (K,)
    name = 'track_step' if api == 'track' else 'track_hands_step'
    if kind == 'f32':
        return getattr(e, name)(fr, hs, *k, want_kpmap=kp)
    if kind == 'u8':
        return getattr(e, name + '_u8')(TO.to_u8(fr), hs, *k, want_kpmap=kp)
    if kind == 'nv12':
        y, uv = NV.rgb_to_nv12(TO.to_u8(fr))
        return getattr(e, name + '_nv12')(y, uv, hs, *k, want_kpmap=kp)
    o = e._track_outputs(B, kp) if api == 'track' else e._track_hands_outputs(B, K, kp)
    return _on_device(e, lambda i, h, **kw: getattr(e, name + '_dev')(B, H, W, *k, i, h, **kw), o, fr, hs)


def run(e, name):
    """Scenario `name` on engine `e` (all weights loaded, float32): {'rows': per step, 'counters': the non-zero deltas, 'digests': per
    step}.  Leaves the options at their defaults and both trackers reset."""
    sc = SCENARIOS[name]
    B, H, W, K = sc['B'], sc['H'], sc['W'], sc['K']
    e.track_reset()
    e.track_hands_reset()
    try:
        for k, v in sc['opts'].items():
            e.set_option(k, v)
        centre = np.array([H / 2.0, W / 2.0], F32)
        if sc['seed'] is not None and sc['api'] == 'track':
            c = np.tile(centre, (B, 1))
            c[np.array(sc['seed'], np.int64)] = FAR
            e.track_seed(c, np.full(B, 10.0, F32), H, W)
        elif sc['seed'] is not None:
            e.track_hands_seed(np.tile(centre, (B, K, 1)), np.full((B, K), 10.0, F32), np.array(sc['seed'], np.int32), H, W)
        n0 = {k: e.counter(k) for k in COUNTERS}
        rows, digests = [], []
        e.set_profiling(sc['prof'])
        for t in range(sc['steps']):
            o = _step(e, sc, t)
            rows.append([r[0] for r in e.profile()])
            digests.append({k: _digest(v) for k, v in sorted(o.items())})
        delta = {k: e.counter(k) - n0[k] for k in COUNTERS}
        return {'rows': rows, 'counters': {k: v for k, v in delta.items() if v}, 'digests': digests}
    finally:
        e.set_profiling(0)
        for k, v in OPTION_DEFAULTS.items():
            e.set_option(k, v)
        e.track_reset()
        e.track_hands_reset()


def plan_engine(lib):
    from hand3d_amd import _lib
    e = _lib.Engine(0, path=lib)
    e.load_weight_dict(synth.make_weights())
    e.finalize_weights(0)
    return e


def expected(section):
    with open(FIXTURE) as f:
        return json.load(f)[section]


def record(lib, names, jobs=1):
    if jobs <= 1:
        e = plan_engine(lib)
        try:
            return {n: run(e, n) for n in names}
        finally:
            e.close()
    tmp = ['%s.part%d' % (os.path.join(HERE, '_cache', 'step_plan'), i) for i in range(jobs)]
    os.makedirs(os.path.dirname(tmp[0]), exist_ok=True)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), '--lib', lib, '--out', tmp[i], '--names', ','.join(names[i::jobs])])
             for i in range(jobs) if names[i::jobs]]
    out = {}
    for i, p in enumerate(procs):
        if p.wait() != 0:
            raise RuntimeError('recorder %d failed' % i)
        with open(tmp[i]) as f:
            out.update(json.load(f))
        os.remove(tmp[i])
    return {n: out[n] for n in names}


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--jobs', type=int, default=1)
    ap.add_argument('--names', default=','.join(SCENARIOS))
    a = ap.parse_args()
    res = record(os.path.abspath(a.lib), [n for n in a.names.split(',') if n], a.jobs)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write('\n')
