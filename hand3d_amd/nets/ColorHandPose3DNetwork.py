"""ColorHandPose3DNetwork -- the reference's call surface on the MI355X engine.

Mirrors nets/ColorHandPose3DNetwork.py:28-99,101-219 of lmb-freiburg/hand3d: same method
names, argument order, return-tuple order, NHWC float32 shapes.  Where the reference built
TF-graph tensors to be evaluated later by `sess.run`, these methods evaluate eagerly on NumPy
arrays through libhp3d.so (hand-written HIP, gfx950).  There is no TensorFlow, no torch and no
CPU fallback behind them.

A script written against the reference changes three lines:
    net = ColorHandPose3DNetwork()
    net.init(None)                                   # was: net.init(sess) after tf.Session()
    outs = net.inference(image_v, hand_side_v, True) # was: sess.run([...6 tensors...], feed_dict)
"""
from __future__ import print_function, unicode_literals

import os
import pickle

import numpy as np

from .._lib import Engine


def read_weight_file(file_name):
    """One weight file -> dict[tf variable name -> ndarray].  `.pickle` is the reference's format (a pickled dict, :50-53);
    `.npz` holds the same keys and arrays (BASELINE.json's wording "loads the existing .npz weights"):
    written by `export_npz` / `pickle_to_npz` below, read without unpickling anything."""
    assert os.path.exists(file_name), "File not found."
    if file_name.endswith('.npz'):
        with np.load(file_name, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    with open(file_name, 'rb') as fi:
        return pickle.load(fi, encoding='latin1')


def load_weight_files(engine, weight_files, exclude_var_list=None, verbose=True):
    """The loading loop of ColorHandPose3DNetwork.init (:50-59) / PosePriorNetwork.init (:47-57):
    read dict[str -> ndarray] (pickle or .npz), drop keys containing any exclude substring, assign by name.
    Returns the merged dict of what was assigned (later files win, like repeated assign ops)."""
    if exclude_var_list is None:
        exclude_var_list = list()
    loaded = dict()
    for file_name in weight_files:
        weight_dict = read_weight_file(file_name)
        weight_dict = {k: v for k, v in weight_dict.items() if not any([x in k for x in exclude_var_list])}
        if len(weight_dict) > 0:
            engine.load_weight_dict(weight_dict)
            loaded.update(weight_dict)
            if verbose:
                print('Loaded %d variables from %s' % (len(weight_dict), file_name))
    engine.finalize_weights()
    return loaded


def save_npz(weight_dict, npz_path):
    """dict[tf variable name -> ndarray] -> one uncompressed .npz with the same keys (C order, the arrays' own dtype: the
    reference's pickles hold float32, and nothing here narrows a file that holds something else)."""
    np.savez(npz_path, **{k: np.ascontiguousarray(v) for k, v in weight_dict.items()})


def pickle_to_npz(weight_files, npz_path, exclude_var_list=None):
    """Converts the reference's weight pickles (one or several, merged in order) into one .npz that `init` accepts."""
    merged = dict()
    for file_name in weight_files:
        d = read_weight_file(file_name)
        merged.update({k: v for k, v in d.items() if not any([x in k for x in (exclude_var_list or [])])})
    save_npz(merged, npz_path)
    return sorted(merged)


class ColorHandPose3DNetwork(object):
    """ Network performing 3D pose estimation of a human hand from a single color image. """

    def __init__(self, device=0, engine=None, keep_weights=False):
        """`keep_weights=True` keeps a host reference to every array `init` assigns, for `export_npz` (off by default: the engine
        owns a packed device copy, a second 140 MB host copy for the lifetime of the object serves nothing else;
        `pickle_to_npz` converts files without a network object)."""
        self.crop_size = 256
        self.num_kp = 21
        self.engine = engine if engine is not None else Engine(device)
        self.keep_weights = bool(keep_weights)
        self.weight_dict = dict()

    def init(self, session=None, weight_files=None, exclude_var_list=None):
        """ Initializes weights from pickled python dictionaries (reference :34-59) or from `.npz` files with the same keys.
            `session` is accepted for call compatibility and ignored. """
        if weight_files is None:
            weight_files = ['./weights/handsegnet-rhd.pickle', './weights/posenet3d-rhd-stb-slr-finetuned.pickle']
        loaded = load_weight_files(self.engine, weight_files, exclude_var_list)
        if self.keep_weights:
            self.weight_dict.update(loaded)

    def init_from_dict(self, weight_dict, dtype=0):
        """Convenience for synthetic weights: the merged content of the weight files.
        dtype='f16' selects the half-precision trunks (BASELINE config 5)."""
        self.engine.load_weight_dict(weight_dict)
        self.engine.finalize_weights(dtype)
        if self.keep_weights:
            self.weight_dict.update(weight_dict)

    def export_npz(self, npz_path):
        """ Writes every variable assigned so far into one `.npz` (keys = TF variable names) that `init` reads back.
            Needs `keep_weights=True` at construction (or use `pickle_to_npz` on the files). """
        assert self.keep_weights, "export_npz needs ColorHandPose3DNetwork(keep_weights=True) (or use pickle_to_npz on the weight files)"
        save_npz(self.weight_dict, npz_path)

    @staticmethod
    def _check_eval(evaluation):
        if not bool(evaluation):
            raise NotImplementedError("inference engine: evaluation=False (dropout active) is a training path")

    def inference(self, image, hand_side, evaluation):
        """ Full pipeline: HandSegNet + PoseNet + PosePrior (reference :61-99).
            Returns hand_scoremap [B,H,W,2], image_crop [B,256,256,3], scale_crop [B,1],
            center [B,2] (row, col), keypoints_scoremap [B,256,256,21], keypoint_coord3d [B,21,3]. """
        self._check_eval(evaluation)
        o = self.engine.infer_full(image, hand_side)
        return o['scoremap'], o['crop'], o['scale'], o['center'], o['kpmap'], o['coord3d']

    def inference_from_uint8(self, image_u8, hand_side, evaluation, net_size=(240, 320)):
        """ Not in the reference class: the scripts' pre-processing (`x/255 - 0.5`, run.py:59 /
            data/BinaryDbReader.py:182, then resize to 240x320, eval_full.py:50) fused in front of
            inference() on the device.  Same 6-tuple as inference(). """
        self._check_eval(evaluation)
        o = self.engine.infer_full_u8(image_u8, hand_side, net_size[0], net_size[1])
        return o['scoremap'], o['crop'], o['scale'], o['center'], o['kpmap'], o['coord3d']

    def inference_keypoints(self, image, hand_side, evaluation):
        """ Not in the reference class: inference() followed by the scripts' host post-processing
            (run.py:72-73: detect_keypoints + trafo_coords, utils/general.py:331-357) evaluated on the device, so
            neither the 5.5 MB/image heat-maps nor the crop travel to the host.  Returns
            keypoint_coord3d [B,21,3] float32, keypoint_hw [B,21,2] float64 (row, col in the input image),
            keypoint_hw_crop [B,21,2] float64 (row, col in the 256x256 crop), scale_crop [B,1], center [B,2]. """
        self._check_eval(evaluation)
        o = self.engine.infer_full(image, hand_side, outputs=('coord3d', 'kp_crop', 'kp_hw', 'scale', 'center'))
        return o['coord3d'], o['kp_hw'], o['kp_crop'].astype(np.float64), o['scale'], o['center']

    def inference_hands(self, image, hand_side, max_hands, evaluation=True, compact=None):
        """ Not in the reference class: inference() for up to `max_hands` (1 ... 4) hands per frame from ONE HandSegNet pass
            (DESIGN.md 4.12).  Hand k of a frame is the k-th object of the detection map in descending peak foreground score;
            hand 0 is inference()'s hand.  `image` float32 [B,H,W,3] (x/255-0.5) or uint8 [B,H,W,3]; `hand_side` [B,K,2], one
            row per slot.  Returns inference()'s tuple with a K axis -- hand_scoremap [B,H,W,2], image_crop [B,K,256,256,3],
            scale_crop [B,K], center [B,K,2], keypoints_scoremap [B,K,256,256,21], keypoint_coord3d [B,K,21,3] -- plus
            valid [B,K] (0: the slot holds no hand; its outputs come from the fall-back crop), area [B,K] (pixels of the hand's
            mask) and keypoint_hw [B,K,21,2] float64 (row, col in the input image).
            `compact` = True / False sets the engine option "hands_compact", which stays set (None: as it is): True runs everything behind the boxes on the slots
            that hold a hand only, and a slot with valid = 0 returns zeros behind its box instead of the fall-back crop's results
            (the call then waits once per chunk for the valid flags). """
        self._check_eval(evaluation)
        self._compact(compact)
        if np.asarray(image).dtype == np.uint8:
            o = self.engine.infer_hands_u8(image, hand_side, max_hands, H=np.shape(image)[1], W=np.shape(image)[2])
        else:
            o = self.engine.infer_hands(image, hand_side, max_hands)
        return (o['scoremap'], o['crop'], o['scale'], o['center'], o['kpmap'], o['coord3d'], o['valid'], o['area'], o['kp_hw'])

    def _compact(self, compact):
        """None leaves the engine option "hands_compact" as it is; the option is written only when the value differs from what this
        object last wrote (every hp3d_set_option drops captured graphs)."""
        if compact is not None and bool(compact) != getattr(self, '_compact_set', None):
            self.engine.set_option('hands_compact', '1' if compact else '0')
            self._compact_set = bool(compact)

    def _detect_scale(self, detect_scale):
        if detect_scale is not None:
            self.engine.set_option('detect_scale', str(int(detect_scale)))

    def _nv12_matrix(self, nv12_matrix):
        if nv12_matrix is not None:
            self.engine.set_option('nv12_matrix', str(nv12_matrix))

    @staticmethod
    def _nv12_planes(image):
        """(y, uv) if `image` is a pair of NV12 planes, None if it is a packed frame.  A tuple always means planes; a list does only
        where it holds two uint8 arrays [B,H,pitch] and [B,H/2,pitch] (any other list is a nested packed frame, as it always was)."""
        if not isinstance(image, (tuple, list)):
            return None
        pair = len(image) == 2 and all(isinstance(p, np.ndarray) and p.dtype == np.uint8 and p.ndim == 3 for p in image)
        if pair and image[0].shape[0] == image[1].shape[0] and image[0].shape[1] == 2 * image[1].shape[1] and image[0].shape[2] == image[1].shape[2]:
            return image[0], image[1]
        if isinstance(image, tuple):
            raise ValueError("image=(y, uv): NV12 planes are two uint8 arrays [B,H,pitch] and [B,H/2,pitch]; got %s"
                             % ", ".join(str(getattr(p, 'shape', type(p).__name__)) for p in image))
        return None

    def _px_frames(self, image, pixel_format):
        """The frames of a call with `pixel_format`: never a pair of NV12 planes."""
        if isinstance(image, tuple) or self._nv12_planes(image) is not None:
            raise ValueError("pixel_format=%r names a packed frame; image=(y, uv) is a pair of NV12 planes" % (pixel_format,))
        return image

    @staticmethod
    def _surfaces(image, pixel_format):
        """(surfaces, formats) where `image` is a list of B separate surfaces -- uint8 arrays [H,W,pixel_bytes] and (y, uv) pairs --
        under `pixel_format`, one name for all of them or a list of B names ('nv12' for a pair); None for every other call."""
        many = isinstance(pixel_format, (list, tuple))
        if many and not isinstance(image, list):
            raise ValueError("pixel_format=%r lists formats; image must then be a list of as many surfaces" % (pixel_format,))
        if pixel_format is None or not isinstance(image, list) or not image:
            return None
        if not many and ColorHandPose3DNetwork._nv12_planes(image) is not None:
            return None          # (a list of the two planes of one NV12 batch under a packed name: _px_frames refuses it, as it always did)
        if not all(isinstance(s, tuple) or (isinstance(s, np.ndarray) and s.ndim == 3) for s in image):
            if many:
                raise ValueError("image: a surface is a uint8 array [H,W,pixel_bytes] or a pair (y, uv) of NV12 planes")
            return None          # (a nested list of numbers: one packed frame, as it always was)
        formats = list(pixel_format) if many else [pixel_format] * len(image)
        if len(formats) != len(image):
            raise ValueError("pixel_format names %d formats, image holds %d surfaces" % (len(formats), len(image)))
        for i, (s, f) in enumerate(zip(image, formats)):
            if isinstance(s, tuple) and f != 'nv12':
                raise ValueError("surface %d: pixel_format=%r names a packed frame; (y, uv) is a pair of NV12 planes" % (i, f))
            if not isinstance(s, tuple) and f == 'nv12':
                raise ValueError("surface %d: pixel_format='nv12' wants a pair (y, uv) of planes, got an array" % i)
        return image, formats

    def track(self, image, hand_side, detect_scale=None, partial_detect=None, nv12_matrix=None, pixel_format=None):
        """ Not in the reference class: inference_keypoints() for the frames of a video.  The first call (and any
            call after track_reset(), a change of the batch or frame size, or a step that lost a hand) detects the hand with
            HandSegNet as inference() does; every other call crops with the box the dataset readers' hand_crop rule
            (data/BinaryDbReader.py:268-308) derives from the previous call's keypoints and runs no HandSegNet at all.
            `image` float32 [B,H,W,3] (x/255-0.5) or uint8 [B,H,W,3] (tracked steps then crop straight from the uint8 frame).
            Returns what inference_keypoints() returns -- keypoint_coord3d, keypoint_hw, keypoint_hw_crop, scale_crop, center (the
            box this step used) -- plus confidence [B], lost [B] (1: the next step will detect again) and detected [B]
            (1: this step's box came from HandSegNet).
            `detect_scale` = f in 1 ... 8 sets the engine option of that name, which stays set (None: as it is): a detect step finds the
            hand on the frame's f x f area mean and crops from the frame itself; the outputs keep their shapes.
            `partial_detect` = True / False sets the engine option "track_partial_detect", which stays set (None: as it is): a step
            that detects because some frames of the batch lost their hand runs HandSegNet on those frames only; the others keep
            their tracked box and come out bit-equal to a step without the option.
            `image` = (y, uv), a tuple or a list of the two arrays: NV12 frames as a decoder delivers them, uint8 planes [B,H,W] and
            [B,H/2,W]; a tuple that is no such pair raises ValueError.  The crop
            and the detection frame come straight from the planes; every output equals the call on the uint8 frame
            hand3d_amd.utils.nv12.nv12_to_rgb makes of them, bit for bit.  `nv12_matrix` = 'bt709' | 'bt601' | 'bt709_full' |
            'bt601_full' sets the engine option of that name, which stays set (None: as it is; a fresh engine has 'bt709').
            `pixel_format` = 'rgb' | 'bgr' | 'rgba' | 'bgra' | 'argb' | 'abgr': `image` is uint8 [B,H,W,3 or 4] in that byte order
             -- what cv2.VideoCapture ('bgr') or a capture surface ('bgra') hands over.  An array whose rows are padded
            to a pitch, or a region of interest of a wider surface, is read as it lies; the fourth byte is ignored.  Every output
            equals the call on the uint8 RGB frame hand3d_amd.utils.pixels.to_rgb makes of it, bit for bit.  ValueError: a last axis
            that does not match the format, frames that are not uint8, an (y, uv) pair.  None: as without the argument.
            `image` = a list of B surfaces with `pixel_format` = one name for all of them or a list of B names: frame b
            of the batch is surface b, an array of its own -- uint8 [H,W,3 or 4] in a packed format, or a pair (y [H,W], uv [H/2,W])
            under the name 'nv12' -- each at its own pitch, the formats mixed freely: one stream per frame.  Every output equals the
            call on the stack hand3d_amd.utils.pixels.surfaces_to_rgb makes of them, bit for bit.  ValueError: a wrong number of
            names, a pair under a packed name, an array under 'nv12'. """
        self._detect_scale(detect_scale)
        self._nv12_matrix(nv12_matrix)
        if partial_detect is not None:
            self.engine.set_option('track_partial_detect', '1' if partial_detect else '0')
        surfaces = self._surfaces(image, pixel_format)
        planes = None if pixel_format is not None else self._nv12_planes(image)
        if surfaces is not None:
            o = self.engine.track_step_surf(surfaces[0], surfaces[1], hand_side)
        elif pixel_format is not None:
            o = self.engine.track_step_px(self._px_frames(image, pixel_format), pixel_format, hand_side)
        elif planes is not None:
            o = self.engine.track_step_nv12(planes[0], planes[1], hand_side)
        else:
            step = self.engine.track_step_u8 if np.asarray(image).dtype == np.uint8 else self.engine.track_step
            o = step(image, hand_side)
        return (o['coord3d'], o['kp_hw'], o['kp_crop'].astype(np.float64), o['scale'], o['center'], o['confidence'], o['lost'],
                o['detected'])

    def track_reset(self):
        """ The next track() call detects the hand anew (a cut in the video, another hand). """
        self.engine.track_reset()

    def track_hands(self, image, hand_side, max_hands, detect_scale=None, compact=None, nv12_matrix=None, partial_detect=None,
                    pixel_format=None):
        """ Not in the reference class: track() for up to `max_hands` (1 ... 4) hands per frame.  Slot k of a frame
            keeps following its hand for as long as it is not lost, so the slot index is the hand's identity from frame to frame.
            A call detects (HandSegNet once per frame) after track_hands_reset() or a change of the batch, slot count or frame size,
            when a followed hand was lost, when a frame has no hand to follow, or on the `track_redetect` schedule; a detect step
            keeps the slots that still follow a hand and fills the free ones with the objects none of them claims.
            `image` float32 [B,H,W,3] (x/255-0.5) or uint8 [B,H,W,3]; `hand_side` [B,K,2], one row per slot.
            Returns track()'s tuple with a K axis plus valid [B,K] (0: the slot holds no hand) and area [B,K] (pixels of the
            object where detected = 1).  The engine's `claimed` counters (objects a kept slot claimed on a detect step) are not in the
            tuple: Engine.track_hands_step returns them.  `detect_scale`: as for track().
            `compact`: as for inference_hands() -- a slot with valid = 0 costs nothing behind its box and returns zeros there and
            confidence = 0; tracked steps add no stream synchronise, detect steps wait once per chunk for the valid flags.
            `image` = (y, uv) and `nv12_matrix`: NV12 frames, as for track().  `pixel_format`: packed 8-bit frames, as for track();
            a list of B surfaces with one name or B names: one surface per frame, formats mixed, as for track().
            `partial_detect` = True / False sets the engine option "track_hands_partial_detect", which stays set (None: as it is): a
            step that detects because some frames of the batch lost a hand (or have none to follow) runs HandSegNet on those frames
            only; every slot of the other frames keeps what it has -- a slot without a hand there is filled by the next scheduled
            (`track_redetect`) or whole detect step, not by this one. """
        self._detect_scale(detect_scale)
        self._compact(compact)
        self._nv12_matrix(nv12_matrix)
        if partial_detect is not None:
            self.engine.set_option('track_hands_partial_detect', '1' if partial_detect else '0')
        surfaces = self._surfaces(image, pixel_format)
        planes = None if pixel_format is not None else self._nv12_planes(image)
        if surfaces is not None:
            o = self.engine.track_hands_step_surf(surfaces[0], surfaces[1], hand_side, max_hands)
        elif pixel_format is not None:
            o = self.engine.track_hands_step_px(self._px_frames(image, pixel_format), pixel_format, hand_side, max_hands)
        elif planes is not None:
            o = self.engine.track_hands_step_nv12(planes[0], planes[1], hand_side, max_hands)
        else:
            step = self.engine.track_hands_step_u8 if np.asarray(image).dtype == np.uint8 else self.engine.track_hands_step
            o = step(image, hand_side, max_hands)
        return (o['coord3d'], o['kp_hw'], o['kp_crop'].astype(np.float64), o['scale'], o['center'], o['confidence'], o['lost'],
                o['detected'], o['valid'], o['area'])

    def track_hands_reset(self):
        """ The next track_hands() call detects anew and keeps no slot. """
        self.engine.track_hands_reset()

    def inference2d_keypoints(self, image):
        """ inference2d() + detect_keypoints + trafo_coords on the device (eval2d.py:58,93-94): keypoint_hw [B,21,2]
            float64 in the input image, keypoint_hw_crop [B,21,2] float64, scale_crop, center. """
        kpc, kph, scale, center = self.engine.infer_2d_keypoints(image)
        return kph, kpc.astype(np.float64), scale, center

    def inference2d(self, image):
        """ Only 2D part of the pipeline: HandSegNet + PoseNet (reference :101-129).
            Returns keypoints_scoremap, image_crop, scale_crop, center -- note the order. """
        return self.engine.infer_2d(image)

    def inference_detection(self, image, train=False):
        """ HandSegNet (reference :131-168).  Returns a list (len 1) of [B,H,W,2] score maps. """
        if train:
            raise NotImplementedError("inference engine: train=True is not supported")
        return [self.engine.handsegnet(image)]

    def inference_pose2d(self, image_crop, train=False):
        """ PoseNet (reference :170-219).  Returns the list of 3 [B,h/8,w/8,21] score maps. """
        if train:
            raise NotImplementedError("inference engine: train=True is not supported")
        return self.engine.posenet2d(image_crop)

    def _inference_pose3d(self, keypoints_scoremap, hand_side, evaluation, train=False):
        """ PosePrior + Viewpoint on a [B,32,32,21] score map (reference :221-247). """
        self._check_eval(evaluation)
        return self.engine.pose3d(keypoints_scoremap, hand_side)[0]
