#!/usr/bin/env python
"""Tracking a hand through the frames of a video on the MI355X engine: the first frame detects the hand with
HandSegNet, every later frame crops with the box derived from the previous frame's keypoints and runs no HandSegNet at all --
until a frame reports the hand as lost, which makes the next one detect again.

    python examples/track.py frames_dir/                  (*.png / *.jpg in name order; needs ./weights/*.pickle, like run.py)
    python examples/track.py frames.npy                   (uint8 or float [N,H,W,3])
    python examples/track.py --synthetic                  (seeded synthetic weights + frames)
    python examples/track.py --synthetic --hands 2        (up to K hands per frame, each in its own slot: DESIGN.md 4.13)
    python examples/track.py video_hd.npy --detect-scale 4   (detect on the 4 x 4 area mean, crop from the frame: DESIGN.md 4.14)
    python examples/track.py batch.npy --hands 2 --partial-detect   (a lost hand costs its own frame's detection only: DESIGN.md 4.18)
    python examples/track.py video_hd.npy --nv12             (the frames as NV12 planes, what a decoder delivers: DESIGN.md 4.17)
    python examples/track.py video_hd.npy --pixel-format bgra   (the frames as packed BGRA, what a capture surface holds: DESIGN.md 4.19)
    python examples/track.py video_hd.npy --surfaces bgra,nv12,bgr   (one batch of three streams -- the video at offsets of one frame --
                                                          each frame a surface of its own in its own format: DESIGN.md 4.20)
"""
import glob
import json
import os
import tempfile

import numpy as np

from common import parser, synthetic_weight_files

if __name__ == '__main__':
    ap = parser(__doc__)
    ap.add_argument('frames', nargs='?')
    ap.add_argument('--redetect', type=int, default=0, help='every N-th frame detects anew (0: only when the hand is lost)')
    ap.add_argument('--hands', type=int, default=0, metavar='K',
                    help='follow up to K hands per frame, each in its own slot (0: the single-hand tracker)')
    ap.add_argument('--detect-scale', type=int, default=1, metavar='F', choices=range(1, 9),
                    help='detect steps find the hand on the F x F area mean of the frame and crop from the frame itself (1: detect on the frame)')
    ap.add_argument('--compact', action='store_true',
                    help='with --hands K: slots without a hand cost nothing behind their box and report zeros (DESIGN.md 4.15)')
    ap.add_argument('--partial-detect', action='store_true',
                    help='a step that detects because some frames of a batch lost their hand runs HandSegNet on those frames only '
                         '(DESIGN.md 4.16; with --hands K: on the frames that lost a hand or have none to follow, DESIGN.md 4.18)')
    ap.add_argument('--nv12', action='store_true',
                    help='convert the loaded frames to NV12 planes and track on those: crop and detection frame come straight from the '
                         'planes (DESIGN.md 4.17; frames with even height and width)')
    ap.add_argument('--nv12-matrix', default='bt709', choices=('bt709', 'bt601', 'bt709_full', 'bt601_full'),
                    help='the colour matrix of --nv12, both ways (default bt709: HD video)')
    ap.add_argument('--pixel-format', default=None, metavar='FMT', choices=('rgb', 'bgr', 'rgba', 'bgra', 'argb', 'abgr'),
                    help='re-lay the loaded frames as packed 8-bit pixels in this byte order and track on those: crop and detection '
                         'frame come straight from them (DESIGN.md 4.19); not with --nv12')
    ap.add_argument('--surfaces', default=None, metavar='FMT0,FMT1,...',
                    help='track a batch of streams, one per listed format cycled over the batch (rgb ... abgr, nv12): stream k shows the '
                         'video k frames ahead, and every frame of the batch is a surface of its own in its format (DESIGN.md 4.20); '
                         'not with --nv12 or --pixel-format')
    ap.add_argument('--min-score', default='off', help='confidence below which a hand counts as lost (calibrate on real weights)')
    ap.add_argument('--float-range', choices=('255', 'normalised'), default='255',
                    help='float frames of a .npy file: 0..255 values (default) or already x/255-0.5')
    a = ap.parse_args()
    if not a.synthetic and not a.frames:
        ap.error('give a directory of frames or a .npy file (or --synthetic)')
    if a.nv12 and a.pixel_format:
        ap.error('--nv12 and --pixel-format name two different frame layouts: give one')
    surf_formats = a.surfaces.split(',') if a.surfaces else []
    if surf_formats and (a.nv12 or a.pixel_format):
        ap.error('--surfaces names the layout of every frame of the batch: not with --nv12 or --pixel-format')
    if any(f not in ('rgb', 'bgr', 'rgba', 'bgra', 'argb', 'abgr', 'nv12') for f in surf_formats):
        ap.error('--surfaces takes rgb, bgr, rgba, bgra, argb, abgr and nv12, separated by commas')
    from hand3d_amd import synth
    from hand3d_amd.nets.ColorHandPose3DNetwork import ColorHandPose3DNetwork

    net = ColorHandPose3DNetwork(device=a.device)
    if a.synthetic:
        net.init(None, weight_files=synthetic_weight_files(tempfile.mkdtemp()))
        base = (synth.make_image(0) + 0.5) * 255.0
        frames = [np.roll(base, 3 * i, axis=1) for i in range(8)]          # the same scene drifting to the right
    else:
        net.init(None, weight_files=['%s/handsegnet-rhd.pickle' % a.weights_dir,
                                     '%s/posenet3d-rhd-stb-slr-finetuned.pickle' % a.weights_dir])
        if a.frames.endswith('.npy'):
            frames = list(np.load(a.frames))
        else:
            try:
                from PIL import Image
            except ImportError:
                ap.error('reading image files needs Pillow; pass the frames as a .npy array instead')
            paths = sorted(p for ext in ('png', 'jpg', 'jpeg') for p in glob.glob(os.path.join(a.frames, '*.' + ext)))
            frames = [np.asarray(Image.open(p).convert('RGB')) for p in paths]
    net.engine.set_option('track_redetect', str(a.redetect))
    net.engine.set_option('track_min_score', a.min_score)
    net.engine.set_option('detect_scale', str(a.detect_scale))
    net.engine.set_option('track_partial_detect', '1' if a.partial_detect else '0')
    net.engine.set_option('track_hands_partial_detect', '1' if a.partial_detect else '0')
    hand_side_v = np.array([[1.0, 0.0]], np.float32)                      # run.py:40: left hand
    net.track_reset()
    net.track_hands_reset()
    nb = max(len(surf_formats), 1)                                       # streams in the batch
    hand_side_v = np.tile(hand_side_v, (nb, 1))
    if a.hands:
        hand_side_v = np.tile(hand_side_v, (1, a.hands, 1)).reshape(nb, a.hands, 2)          # which slot holds a left hand is the caller's knowledge
    if a.nv12 or 'nv12' in surf_formats:
        from hand3d_amd.utils.nv12 import rgb_to_nv12
        net.engine.set_option('nv12_matrix', a.nv12_matrix)
    if a.pixel_format or surf_formats:
        from hand3d_amd.utils.pixels import from_rgb
    track_kw = {'pixel_format': a.pixel_format} if a.pixel_format else {'pixel_format': surf_formats} if surf_formats else {}

    def as_u8(frame):
        if frame.dtype != np.uint8:
            frame = (frame + 0.5) * 255.0 if a.float_range == 'normalised' else frame
            frame = np.clip(np.floor(np.asarray(frame, np.float64) + 0.5), 0, 255).astype(np.uint8)
        return frame

    for i, frame in enumerate(frames):
        frame = np.asarray(frame)
        if surf_formats:               # stream k: the video k frames ahead, as a surface of its own in format k
            image_v = []
            for k, fmt in enumerate(surf_formats):
                u8 = as_u8(np.asarray(frames[(i + k) % len(frames)]))[None]
                image_v.append(tuple(p[0] for p in rgb_to_nv12(u8, a.nv12_matrix)) if fmt == 'nv12' else from_rgb(u8, fmt)[0])
        elif a.nv12 or a.pixel_format:   # (a video source hands its frames over as they are; here they are made from the loaded frame)
            frame = as_u8(frame)
            image_v = rgb_to_nv12(frame[None], a.nv12_matrix) if a.nv12 else from_rgb(frame[None], a.pixel_format)
        elif frame.dtype == np.uint8:
            image_v = frame[None]                      # tracked steps crop straight from the uint8 frame
        elif a.float_range == '255':
            image_v = frame[None].astype(np.float32) / 255.0 - 0.5
        else:
            image_v = frame[None].astype(np.float32)
        ndet = net.engine.counter('track_hands_detect_steps')
        if a.hands:
            coord3d, kp_hw, _, scale, center, confidence, lost, detected, valid, area = net.track_hands(image_v, hand_side_v, a.hands, compact=a.compact,
                                                                                               **track_kw)
            for b in range(nb):
                print(json.dumps(dict({'frame': i, 'step': 'detect' if net.engine.counter('track_hands_detect_steps') > ndet else 'tracked',
                                       'slots': [{'slot': k, 'valid': int(valid[b, k]), 'detected': int(detected[b, k]), 'area': int(area[b, k]),
                                                  'center': center[b, k].tolist(), 'scale': float(scale[b, k]),
                                                  'confidence': float(confidence[b, k]), 'lost': int(lost[b, k]),
                                                  'wrist_hw': kp_hw[b, k, 0].tolist(), 'wrist_xyz': coord3d[b, k, 0].tolist()}
                                                 for k in range(a.hands)]}, **({'stream': b, 'format': surf_formats[b]} if surf_formats else {}))))
            continue
        coord3d, kp_hw, kp_hw_crop, scale, center, confidence, lost, detected = net.track(image_v, hand_side_v, **track_kw)
        for b in range(nb):
            print(json.dumps(dict({'frame': i, 'step': 'detect' if detected[b] else 'tracked', 'center': center[b].tolist(),
                                   'scale': float(scale[b, 0]), 'confidence': float(confidence[b]), 'lost': int(lost[b]),
                                   'wrist_hw': kp_hw[b, 0].tolist(), 'wrist_xyz': coord3d[b, 0].tolist()},
                                  **({'stream': b, 'format': surf_formats[b]} if surf_formats else {}))))
