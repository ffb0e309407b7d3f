"""ctypes binding of libhp3d.so (include/hp3d.h) -- the only bridge between the Python call
surface and the HIP engine.  No torch, no numpy fallback: if the library is missing or no GPU is
visible, the product path raises.

HP3D_LIB=<path> overrides the library (the CPU test-suite points it at tests/emu/libhp3d_emu.so,
an interpreter of the same kernel sources; see tests/emu/hp3d_emu.h).
"""
import ctypes as C
import os
import weakref

import numpy as np

from .utils.pixels import FORMATS, SURF_NV12

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, 'libhp3d.so')

VARIANTS = {'direct': 0, 'bottleneck': 1, 'proposed': 2, 'local': 3, 'local_w_xyz_loss': 3}
NET_SEG, NET_POSE, NET_PRIOR, NET_VP, NET_BOTTLENECK = 1, 2, 4, 8, 16

_f = C.POINTER(C.c_float)
_i32 = C.POINTER(C.c_int32)
_ctx = C.c_void_p

_SIGNATURES = {
    'hp3d_abi_version': (C.c_int, []),
    'hp3d_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'hp3d_device_pci_bus_id': (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    'hp3d_create': (C.c_int, [C.c_int, C.POINTER(_ctx)]),
    'hp3d_destroy': (C.c_int, [_ctx]),
    'hp3d_last_error': (C.c_char_p, [_ctx]),
    'hp3d_stream': (C.c_void_p, [_ctx]),
    'hp3d_sync': (C.c_int, [_ctx]),
    'hp3d_set_option': (C.c_int, [_ctx, C.c_char_p, C.c_char_p]),
    'hp3d_set_weight': (C.c_int, [_ctx, C.c_char_p, _f, C.POINTER(C.c_int64), C.c_int]),
    'hp3d_finalize_weights': (C.c_int, [_ctx, C.c_int]),
    'hp3d_weights_blob_bytes': (C.c_int, [_ctx, C.POINTER(C.c_size_t)]),
    'hp3d_weights_blob_export': (C.c_int, [_ctx, C.c_void_p]),
    'hp3d_weights_blob_import': (C.c_int, [_ctx, C.c_void_p, C.c_int]),
    'hp3d_nets_mask': (C.c_int, [_ctx]),
    'hp3d_infer_full': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9),
    'hp3d_infer_full_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9),
    'hp3d_infer_full_kp': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    'hp3d_infer_full_kp_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    'hp3d_infer_full_kp_u8': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10),
    'hp3d_infer_full_u8': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8),
    'hp3d_preprocess_u8': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_infer_2d': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5),
    'hp3d_infer_2d_kp': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7),
    'hp3d_detect_keypoints': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_handsegnet': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3),
    'hp3d_posenet2d': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4),
    'hp3d_posenet2d_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4),
    'hp3d_poseprior': (C.c_int, [_ctx, C.c_int, C.c_int] + [C.c_void_p] * 5),
    'hp3d_pose3d': (C.c_int, [_ctx, C.c_int] + [C.c_void_p] * 5),
    'hp3d_conv2d': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_conv2d_f16': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_first_block_f16': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5),
    'hp3d_maxpool2': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_avgpool8': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_resize_bilinear': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_crop_and_resize': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p]),
    'hp3d_infer_hands': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13),
    'hp3d_infer_hands_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13),
    'hp3d_infer_hands_u8': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 12),
    'hp3d_masks_from_scoremap': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7),
    'hp3d_masks_from_scoremap_keep': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    'hp3d_track_hands_reset': (C.c_int, [_ctx]),
    'hp3d_track_hands_seed': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hp3d_track_hands_step': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 15),
    'hp3d_track_hands_step_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 15),
    'hp3d_track_hands_step_u8': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 14),
    'hp3d_track_hands_box': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 7),
    'hp3d_track_reset': (C.c_int, [_ctx]),
    'hp3d_track_seed': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'hp3d_track_step': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 12),
    'hp3d_track_step_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 12),
    'hp3d_track_step_nv12': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 11),
    'hp3d_track_step_nv12_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 11),
    'hp3d_track_hands_step_nv12': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 14),
    'hp3d_track_hands_step_nv12_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 14),
    'hp3d_nv12_to_rgb': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    'hp3d_crop_and_resize_nv12': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_downscale_nv12': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                      C.c_int, C.c_void_p]),
    'hp3d_track_step_px': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 11),
    'hp3d_track_step_px_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 11),
    'hp3d_track_hands_step_px': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 14),
    'hp3d_track_hands_step_px_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 14),
    'hp3d_px_to_rgb': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    'hp3d_crop_and_resize_px': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_downscale_px': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p]),
    'hp3d_track_step_surf': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_void_p] * 11),
    'hp3d_track_step_surf_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_void_p] * 11),
    'hp3d_track_hands_step_surf': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 14),
    'hp3d_track_hands_step_surf_dev': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 14),
    'hp3d_surf_to_rgb': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_crop_and_resize_surf': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_int, C.c_void_p]),
    'hp3d_downscale_surf': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'hp3d_track_step_u8': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 11),
    'hp3d_track_box': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 4),
    'hp3d_crop_and_resize_u8': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'hp3d_crop_and_resize_idx': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_slot_scatter': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_downscale': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_downscale_u8': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_gather_frames': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'hp3d_track_hands_partial_index': (C.c_int, [_ctx, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.c_int32)]),
    'hp3d_track_hands_select_pos': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13),
    'hp3d_boxes_to_frame': (C.c_int, [_ctx, C.c_int, C.c_int] + [C.c_void_p] * 5),
    'hp3d_boxes_to_detect': (C.c_int, [_ctx, C.c_int, C.c_int] + [C.c_void_p] * 4),
    'hp3d_mask_from_scoremap': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5),
    'hp3d_fc': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_argmax2d': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_dev_alloc': (C.c_int, [_ctx, C.c_size_t, C.POINTER(C.c_void_p)]),
    'hp3d_dev_free': (C.c_int, [_ctx, C.c_void_p]),
    'hp3d_host_alloc': (C.c_int, [_ctx, C.c_size_t, C.POINTER(C.c_void_p)]),
    'hp3d_host_free': (C.c_int, [_ctx, C.c_void_p]),
    'hp3d_memcpy': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    'hp3d_upload_async': (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_size_t]),
    'hp3d_wait_upload': (C.c_int, [_ctx]),
    'hp3d_get_counter': (C.c_int, [_ctx, C.c_char_p, C.POINTER(C.c_longlong)]),
    'hp3d_set_profiling': (C.c_int, [_ctx, C.c_int]),
    'hp3d_prof_count': (C.c_int, [_ctx]),
    'hp3d_prof_get': (C.c_int, [_ctx, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_float),
                                C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'hp3d_get_timing': (C.c_int, [_ctx, C.POINTER(C.c_float), C.c_int]),
    'hp3d_comm_unique_id': (C.c_int, [C.c_void_p]),
    'hp3d_comm_init': (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p]),
    'hp3d_bcast_weights': (C.c_int, [_ctx, C.c_int]),
    'hp3d_allgather': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_void_p]),
    'hp3d_allgather_dev': (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_void_p]),
    'hp3d_comm_destroy': (C.c_int, [_ctx]),
    'hp3d_crc32c': (C.c_uint32, [C.c_void_p, C.c_size_t]),
}
COMM_ID_BYTES = 128
MAX_HANDS = 4               # HP3D_MAX_HANDS
TIMING_STAGES = ('HandSegNet', 'mask_crop', 'PoseNet2D', 'lifting', 'total')
EXPORTS = tuple(sorted(_SIGNATURES))


class Surface(C.Structure):
    """hp3d_surface of include/hp3d.h: one frame of a batch of separate surfaces."""
    _fields_ = [('data', C.c_void_p), ('chroma', C.c_void_p), ('pitch', C.c_int32), ('format', C.c_int32), ('height', C.c_int32),
                ('width', C.c_int32)]

_lib = None
_lib_path = None
_loaded = {}


class Hp3dError(RuntimeError):
    pass


def lib_path():
    return os.environ.get('HP3D_LIB', DEFAULT_LIB)


def load(path=None):
    """dlopen the engine and attach prototypes.  Raises if the library is absent: there is no
    Python/NumPy fallback for the product path."""
    global _lib, _lib_path
    path = os.path.abspath(path or lib_path())
    if path in _loaded:
        return _loaded[path]
    if not os.path.exists(path):
        raise Hp3dError("HIP engine library not found at %s -- build it with `python -m hand3d_amd.build` "
                        "(hipcc, gfx950). The product has no CPU fallback." % path)
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if include/hp3d.h and the library disagree
        fn.restype = res
        fn.argtypes = args
    _loaded[path] = lib
    _lib, _lib_path = lib, path
    return lib


def device_count(path=None):
    """HIP devices visible to this process (hp3d_device_count); 0 when the runtime reports an error (no GPU, no driver)."""
    n = C.c_int(0)
    rc = load(path).hp3d_device_count(C.byref(n))
    return int(n.value) if rc == 0 else 0


def device_pci_bus_id(device, path=None):
    """PCI address 'dddd:bb:dd.f' of HIP device `device` (hp3d_device_pci_bus_id); raises Hp3dError when the runtime has none."""
    buf = C.create_string_buffer(32)
    rc = load(path).hp3d_device_pci_bus_id(int(device), buf, 32)
    if rc != 0:
        raise Hp3dError('hp3d_device_pci_bus_id(%d) failed: %d' % (device, rc))
    return buf.value.decode()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class DevBuf(object):
    """A device allocation owned through the C ABI (hp3d_dev_alloc / hp3d_dev_free); int(buf) is the device address."""

    def __init__(self, engine, ptr, nbytes):
        self.engine, self.ptr, self.nbytes = engine, ptr, nbytes
        if engine is not None and hasattr(engine, '_devbufs'):
            engine._devbufs.add(self)         # Engine.close() releases whatever is still alive (ptr becomes 0)

    def __int__(self):
        return self.ptr

    def __index__(self):
        return self.ptr

    def at(self, offset_bytes):
        return self.ptr + int(offset_bytes)

    def free(self):
        if self.ptr and self.engine is not None and self.engine.h:
            self.engine.lib.hp3d_dev_free(self.engine.h, C.c_void_p(self.ptr))
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine(object):
    """One hp3d_ctx: a device, a stream, packed weights and a pre-allocated arena."""

    def __init__(self, device=0, path=None):
        self.lib = load(path)
        h = _ctx()
        rc = self.lib.hp3d_create(int(device), C.byref(h))
        if rc != 0:
            raise Hp3dError("hp3d_create(%d) failed: %s" % (device, self.lib.hp3d_last_error(None).decode()))
        self.h = h
        self.device = device
        self._pinned = []
        self._devbufs = weakref.WeakSet()

    def close(self):
        """Destroys the context.  Device buffers handed out by dev_alloc / to_device that are still alive are freed here
        (their `ptr` becomes 0), and so are the page-locked buffers behind pinned_empty(): arrays returned by pinned_empty()
        must not be touched after close() -- hp3d_host_free waits for pending uploads first."""
        if getattr(self, 'h', None):
            for b in list(getattr(self, '_devbufs', [])):
                b.free()
            for p in getattr(self, '_pinned', []):
                self.lib.hp3d_host_free(self.h, C.c_void_p(p))
            self._pinned = []
            self.lib.hp3d_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.hp3d_last_error(self.h).decode()
            if rc == -1:
                raise AssertionError(msg)            # the reference's bare asserts
            if rc == -4:
                raise NotImplementedError(msg)
            raise Hp3dError("hp3d error %d: %s" % (rc, msg))

    # -- options / weights -------------------------------------------------------------------
    def set_option(self, key, value):
        self._chk(self.lib.hp3d_set_option(self.h, key.encode(), value.encode()))

    def set_weight(self, name, array):
        a = _f32(array)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        self._chk(self.lib.hp3d_set_weight(self.h, name.encode(), a.ctypes.data_as(_f), shape, a.ndim))

    def load_weight_dict(self, weight_dict):
        for k in sorted(weight_dict):
            self.set_weight(k, weight_dict[k])

    def finalize_weights(self, dtype=0):
        """dtype 0 = float32; 1 (or 'f16') = half-precision HandSegNet / PoseNet2D trunks (BASELINE config 5)."""
        dtype = {'f32': 0, 'f16': 1}.get(dtype, dtype)
        self._chk(self.lib.hp3d_finalize_weights(self.h, int(dtype)))

    def nets_mask(self):
        return self.lib.hp3d_nets_mask(self.h)

    def blob_bytes(self):
        n = C.c_size_t()
        self._chk(self.lib.hp3d_weights_blob_bytes(self.h, C.byref(n)))
        return n.value

    def blob_export(self, dev_ptr):
        self._chk(self.lib.hp3d_weights_blob_export(self.h, C.c_void_p(dev_ptr)))

    def blob_import(self, dev_ptr, nets_mask):
        self._chk(self.lib.hp3d_weights_blob_import(self.h, C.c_void_p(dev_ptr), int(nets_mask)))

    def sync(self):
        self._chk(self.lib.hp3d_sync(self.h))

    def stream(self):
        return self.lib.hp3d_stream(self.h)

    # -- whole-path --------------------------------------------------------------------------
    def infer_full(self, image, hand_side, want_mask=False, outputs=('scoremap', 'crop', 'scale', 'center', 'kpmap', 'coord3d')):
        image, hand_side = _f32(image), _f32(hand_side)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        assert hand_side.shape == (B, 2), "hand_side must be [B,2]"
        o = {
            'scoremap': np.empty((B, H, W, 2), np.float32) if 'scoremap' in outputs else None,
            'crop': np.empty((B, 256, 256, 3), np.float32) if 'crop' in outputs else None,
            'scale': np.empty((B, 1), np.float32) if 'scale' in outputs else None,
            'center': np.empty((B, 2), np.float32) if 'center' in outputs else None,
            'kpmap': np.empty((B, 256, 256, 21), np.float32) if 'kpmap' in outputs else None,
            'coord3d': np.empty((B, 21, 3), np.float32) if 'coord3d' in outputs else None,
            'mask': np.empty((B, H, W), np.float32) if want_mask else None,
            # detect_keypoints / trafo_coords on the device (utils/general.py:331-357): int32 (row, col) in the crop and
            # float64 (row, col) in the image; need no 'kpmap'
            'kp_crop': np.empty((B, 21, 2), np.int32) if 'kp_crop' in outputs else None,
            'kp_hw': np.empty((B, 21, 2), np.float64) if 'kp_hw' in outputs else None,
        }
        self._chk(self.lib.hp3d_infer_full_kp(self.h, B, H, W, _ptr(image), _ptr(hand_side), _ptr(o['scoremap']),
                                              _ptr(o['crop']), _ptr(o['scale']), _ptr(o['center']), _ptr(o['kpmap']),
                                              _ptr(o['coord3d']), _ptr(o['mask']), _ptr(o['kp_crop']), _ptr(o['kp_hw'])))
        return o

    def infer_full_u8(self, image_u8, hand_side, H=240, W=320, want_mask=False):
        """uint8 frames [B,Hin,Win,3] -> normalise + resize on device -> full pipeline."""
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        hand_side = _f32(hand_side)
        assert img.ndim == 4 and img.shape[3] == 3, "image must be [B,Hin,Win,3] uint8"
        B, Hin, Win, _ = img.shape
        assert hand_side.shape == (B, 2), "hand_side must be [B,2]"
        o = {'scoremap': np.empty((B, H, W, 2), np.float32), 'crop': np.empty((B, 256, 256, 3), np.float32),
             'scale': np.empty((B, 1), np.float32), 'center': np.empty((B, 2), np.float32),
             'kpmap': np.empty((B, 256, 256, 21), np.float32), 'coord3d': np.empty((B, 21, 3), np.float32),
             'mask': np.empty((B, H, W), np.float32) if want_mask else None}
        self._chk(self.lib.hp3d_infer_full_u8(self.h, B, Hin, Win, _ptr(img), H, W, _ptr(hand_side), _ptr(o['scoremap']),
                                              _ptr(o['crop']), _ptr(o['scale']), _ptr(o['center']), _ptr(o['kpmap']),
                                              _ptr(o['coord3d']), _ptr(o['mask'])))
        return o

    def preprocess_u8(self, image_u8, H, W):
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        B, Hin, Win, _ = img.shape
        out = np.empty((B, H, W, 3), np.float32)
        self._chk(self.lib.hp3d_preprocess_u8(self.h, _ptr(img), B, Hin, Win, H, W, _ptr(out)))
        return out

    def infer_full_dev(self, B, H, W, image_ptr, hand_side_ptr, scoremap=0, crop=0, scale=0, center=0, kpmap=0,
                       coord3d=0, mask=0, kp_crop=0, kp_hw=0):
        """Device-pointer variant (ints); stream-ordered, call sync() before reading.  kp_crop (int32 [B,21,2]) /
        kp_hw (float64 [B,21,2]): detect_keypoints / trafo_coords evaluated on the device."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        if kp_crop or kp_hw:
            self._chk(self.lib.hp3d_infer_full_kp_dev(self.h, B, H, W, v(image_ptr), v(hand_side_ptr), v(scoremap), v(crop),
                                                      v(scale), v(center), v(kpmap), v(coord3d), v(mask), v(kp_crop), v(kp_hw)))
        else:
            self._chk(self.lib.hp3d_infer_full_dev(self.h, B, H, W, v(image_ptr), v(hand_side_ptr), v(scoremap), v(crop),
                                                   v(scale), v(center), v(kpmap), v(coord3d), v(mask)))

    # -- several hands per frame (include/hp3d.h) ---------------------------------------
    _HANDS_ORDER = ('scoremap', 'crop', 'scale', 'center', 'kpmap', 'coord3d', 'mask', 'kp_crop', 'kp_hw', 'valid', 'area')
    _HANDS_DEFAULT = ('scoremap', 'crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw')

    @staticmethod
    def _hands_outputs(B, K, H, W, want_mask, outputs):
        want = lambda k: k in outputs
        return {'scoremap': np.empty((B, H, W, 2), np.float32) if want('scoremap') else None,
                'crop': np.empty((B, K, 256, 256, 3), np.float32) if want('crop') else None,
                'scale': np.empty((B, K), np.float32) if want('scale') else None,
                'center': np.empty((B, K, 2), np.float32) if want('center') else None,
                'kpmap': np.empty((B, K, 256, 256, 21), np.float32) if want('kpmap') else None,
                'coord3d': np.empty((B, K, 21, 3), np.float32) if want('coord3d') else None,
                'mask': np.empty((B, K, H, W), np.float32) if want_mask else None,
                'kp_crop': np.empty((B, K, 21, 2), np.int32) if want('kp_crop') else None,
                'kp_hw': np.empty((B, K, 21, 2), np.float64) if want('kp_hw') else None,
                'valid': np.empty((B, K), np.int32), 'area': np.empty((B, K), np.int32)}

    def infer_hands(self, image, hand_side, max_hands, want_mask=False, outputs=_HANDS_DEFAULT):
        """Up to max_hands hands per frame from one HandSegNet pass: image [B,H,W,3], hand_side [B,K,2] (per slot).  Returns a dict with
        infer_full's outputs on an extra K axis ([B,K,...]; scoremap stays [B,H,W,2]) plus valid [B,K] and area [B,K]; slots without a
        hand have valid = 0 and run on the fall-back crop."""
        image, hand_side = _f32(image), _f32(hand_side)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        K = int(max_hands)
        assert hand_side.shape == (B, K, 2), "hand_side must be [B,max_hands,2]"
        o = self._hands_outputs(B, K, H, W, want_mask, outputs)
        self._chk(self.lib.hp3d_infer_hands(self.h, B, H, W, K, _ptr(image), _ptr(hand_side), *[_ptr(o[k]) for k in self._HANDS_ORDER]))
        return o

    def infer_hands_u8(self, image_u8, hand_side, max_hands, H=240, W=320, want_mask=False, outputs=_HANDS_DEFAULT):
        """infer_hands on uint8 frames [B,Hin,Win,3]: normalised and resized to H x W on the device."""
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        hand_side = _f32(hand_side)
        assert img.ndim == 4 and img.shape[3] == 3, "image must be [B,Hin,Win,3] uint8"
        B, Hin, Win, _ = img.shape
        K = int(max_hands)
        assert hand_side.shape == (B, K, 2), "hand_side must be [B,max_hands,2]"
        o = self._hands_outputs(B, K, H, W, want_mask, outputs)
        self._chk(self.lib.hp3d_infer_hands_u8(self.h, B, Hin, Win, _ptr(img), int(H), int(W), K, _ptr(hand_side),
                                               *[_ptr(o[k]) for k in self._HANDS_ORDER]))
        return o

    def infer_hands_dev(self, B, H, W, K, image_ptr, hand_side_ptr, scoremap=0, crop=0, scale=0, center=0, kpmap=0, coord3d=0, mask=0,
                        kp_crop=0, kp_hw=0, valid=0, area=0):
        """Device-pointer variant (ints); stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.lib.hp3d_infer_hands_dev(self.h, B, H, W, K, v(image_ptr), v(hand_side_ptr), v(scoremap), v(crop), v(scale),
                                                v(center), v(kpmap), v(coord3d), v(mask), v(kp_crop), v(kp_hw), v(valid), v(area)))

    def masks_from_scoremap(self, scoremap, max_hands, keep=None):
        """The mask stage of infer_hands alone: scoremap [B,H,W,2] -> dict of mask [B,K,H,W], center [B,K,2], crop_size [B,K],
        scale [B,K], seed int32 [B,K,2], valid [B,K], area [B,K].  keep = (keep [B,K], center [B,K,2], scale [B,K]): the mask stage of a
        multi-hand tracker's detect step -- objects a kept slot claims are dropped and counted in the extra output
        claimed [B,K], the others fill the free slots, kept slots come back as absent ones."""
        sm = _f32(scoremap)
        B, H, W, c2 = sm.shape
        assert c2 == 2
        K = int(max_hands)
        o = {'mask': np.empty((B, K, H, W), np.float32), 'center': np.empty((B, K, 2), np.float32),
             'crop_size': np.empty((B, K), np.float32), 'scale': np.empty((B, K), np.float32),
             'seed': np.empty((B, K, 2), np.int32), 'valid': np.empty((B, K), np.int32), 'area': np.empty((B, K), np.int32)}
        outs = [_ptr(o[k]) for k in ('mask', 'center', 'crop_size', 'scale', 'seed', 'valid', 'area')]
        if keep is None:
            self._chk(self.lib.hp3d_masks_from_scoremap(self.h, _ptr(sm), B, H, W, K, *outs))
            return o
        kk = np.ascontiguousarray(keep[0], dtype=np.int32)
        kc, ks = _f32(keep[1]), _f32(keep[2])
        assert kk.shape == (B, K) and kc.shape == (B, K, 2) and ks.shape == (B, K), "keep must be ([B,K], [B,K,2], [B,K])"
        o['claimed'] = np.empty((B, K), np.int32)
        self._chk(self.lib.hp3d_masks_from_scoremap_keep(self.h, _ptr(sm), B, H, W, K, _ptr(kk), _ptr(kc), _ptr(ks), *outs, _ptr(o['claimed'])))
        return o

    # -- tracking several hands per frame (include/hp3d.h) ------------------------------
    _TRACK_HANDS_ORDER = ('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw', 'confidence', 'lost', 'detected', 'valid',
                          'area', 'claimed')

    @staticmethod
    def _track_hands_outputs(B, K, want_kpmap):
        i32 = lambda: np.empty((B, K), np.int32)
        return {'crop': np.empty((B, K, 256, 256, 3), np.float32), 'scale': np.empty((B, K), np.float32),
                'center': np.empty((B, K, 2), np.float32),
                'kpmap': np.empty((B, K, 256, 256, 21), np.float32) if want_kpmap else None,
                'coord3d': np.empty((B, K, 21, 3), np.float32), 'kp_crop': np.empty((B, K, 21, 2), np.int32),
                'kp_hw': np.empty((B, K, 21, 2), np.float64), 'confidence': np.empty((B, K), np.float32),
                'lost': i32(), 'detected': i32(), 'valid': i32(), 'area': i32(), 'claimed': i32()}

    def track_hands_reset(self):
        """The next track_hands_step detects and keeps no slot."""
        self._chk(self.lib.hp3d_track_hands_reset(self.h))

    def track_hands_seed(self, center, scale, valid, H, W):
        """Start from boxes the caller has: center [B,K,2] (row, col), scale [B,K], valid [B,K] (at least one valid slot per image);
        the next step at (B, K, H, W) is a tracked one."""
        center, scale = _f32(center), _f32(scale)
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        assert scale.ndim == 2, "scale must be [B,K]"
        B, K = scale.shape
        assert center.shape == (B, K, 2) and valid.shape == (B, K), "center must be [B,K,2], valid [B,K]"
        self._chk(self.lib.hp3d_track_hands_seed(self.h, B, int(H), int(W), K, _ptr(center), _ptr(scale), _ptr(valid)))

    def track_hands_step(self, image, hand_side, max_hands, want_kpmap=False):
        """One video step with max_hands slots per frame on float32 frames [B,H,W,3], hand_side [B,K,2].  Returns a dict of [B,K,...]
        arrays: track_step's outputs per slot plus valid, area (pixel count where detected = 1) and claimed (objects the slot claimed
        on a detect step).  The slot index is the hand's identity for as long as the slot is not lost."""
        image, hand_side = _f32(image), _f32(hand_side)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        K = int(max_hands)
        assert hand_side.shape == (B, K, 2), "hand_side must be [B,max_hands,2]"
        o = self._track_hands_outputs(B, K, want_kpmap)
        self._chk(self.lib.hp3d_track_hands_step(self.h, B, H, W, K, _ptr(image), _ptr(hand_side),
                                                 *[_ptr(o[k]) for k in self._TRACK_HANDS_ORDER]))
        return o

    def track_hands_step_u8(self, image_u8, hand_side, max_hands, H=None, W=None, want_kpmap=False):
        """track_hands_step on uint8 frames [B,Hin,Win,3]; tracked steps crop straight from them.  (H, W) default to the frame size,
        the only size the engine accepts here."""
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        hand_side = _f32(hand_side)
        assert img.ndim == 4 and img.shape[3] == 3, "image must be [B,Hin,Win,3] uint8"
        B, Hin, Win, _ = img.shape
        K = int(max_hands)
        assert hand_side.shape == (B, K, 2), "hand_side must be [B,max_hands,2]"
        o = self._track_hands_outputs(B, K, want_kpmap)
        self._chk(self.lib.hp3d_track_hands_step_u8(self.h, B, Hin, Win, _ptr(img), int(H or Hin), int(W or Win), K, _ptr(hand_side),
                                                    *[_ptr(o[k]) for k in self._TRACK_HANDS_ORDER]))
        return o

    def track_hands_step_dev(self, B, H, W, K, image_ptr, hand_side_ptr, crop=0, scale=0, center=0, kpmap=0, coord3d=0, kp_crop=0,
                             kp_hw=0, confidence=0, lost=0, detected=0, valid=0, area=0, claimed=0):
        """Device-pointer variant (ints); stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.lib.hp3d_track_hands_step_dev(self.h, B, H, W, K, v(image_ptr), v(hand_side_ptr), v(crop), v(scale), v(center),
                                                     v(kpmap), v(coord3d), v(kp_crop), v(kp_hw), v(confidence), v(lost), v(detected),
                                                     v(valid), v(area), v(claimed)))

    def track_hands_box(self, keypoint_hw, valid, box_center, box_scale, H, W, score32=None, margin=None):
        """track_box per slot with valid gating: keypoint_hw [B,K,21,2], valid [B,K], the boxes the slots cropped with ([B,K,2], [B,K])
        -> (center [B,K,2], scale [B,K], confidence [B,K], lost [B,K]); an absent slot holds its box with lost = 0."""
        kp = np.ascontiguousarray(keypoint_hw, dtype=np.float64)
        assert kp.ndim == 4 and kp.shape[2:] == (21, 2), "keypoint_hw must be [B,K,21,2]"
        B, K = kp.shape[:2]
        sm = None if score32 is None else _f32(score32)
        assert sm is None or sm.shape == (B, K, 32, 32, 21), "score32 must be [B,K,32,32,21]"
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        bc, bs = _f32(box_center), _f32(box_scale)
        assert valid.shape == (B, K) and bc.shape == (B, K, 2) and bs.shape == (B, K)
        center, scale = np.empty((B, K, 2), np.float32), np.empty((B, K), np.float32)
        conf, lost = np.empty((B, K), np.float32), np.empty((B, K), np.int32)
        assert margin is None or margin > 0, "margin must be positive"
        self._chk(self.lib.hp3d_track_hands_box(self.h, B, K, int(H), int(W), _ptr(kp), _ptr(sm), 0.0 if margin is None else float(margin),
                                                _ptr(valid), _ptr(bc), _ptr(bs), _ptr(center), _ptr(scale), _ptr(conf), _ptr(lost)))
        return center, scale, conf, lost

    # -- tracking: a hand across video frames (include/hp3d.h) -------------------------
    def track_reset(self):
        """The next track_step detects (HandSegNet) whatever the previous step found."""
        self._chk(self.lib.hp3d_track_reset(self.h))

    def track_seed(self, center, scale, H, W):
        """Start from boxes the caller has: center [B,2] (row, col), scale [B]; the next step at (B, H, W) is a tracked one."""
        center, scale = _f32(center), _f32(scale).reshape(-1)
        B = scale.shape[0]
        assert center.shape == (B, 2), "center must be [B,2]"
        self._chk(self.lib.hp3d_track_seed(self.h, B, int(H), int(W), _ptr(center), _ptr(scale)))

    @staticmethod
    def _track_outputs(B, want_kpmap):
        return {'crop': np.empty((B, 256, 256, 3), np.float32), 'scale': np.empty((B, 1), np.float32),
                'center': np.empty((B, 2), np.float32),
                'kpmap': np.empty((B, 256, 256, 21), np.float32) if want_kpmap else None,
                'coord3d': np.empty((B, 21, 3), np.float32), 'kp_crop': np.empty((B, 21, 2), np.int32),
                'kp_hw': np.empty((B, 21, 2), np.float64), 'confidence': np.empty((B,), np.float32),
                'lost': np.empty((B,), np.int32), 'detected': np.empty((B,), np.int32)}

    _TRACK_ORDER = ('crop', 'scale', 'center', 'kpmap', 'coord3d', 'kp_crop', 'kp_hw', 'confidence', 'lost', 'detected')

    def track_step(self, image, hand_side, want_kpmap=False):
        """One video step on float32 frames [B,H,W,3]: a detect step (HandSegNet) or a tracked step (crop from the previous step's
        keypoints).  Returns a dict: crop, scale, center (the boxes this step used), kpmap (or None), coord3d, kp_crop, kp_hw,
        confidence, lost (about the NEXT box), detected (1 where this step's box came from HandSegNet)."""
        image, hand_side = _f32(image), _f32(hand_side)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        assert hand_side.shape == (B, 2), "hand_side must be [B,2]"
        o = self._track_outputs(B, want_kpmap)
        self._chk(self.lib.hp3d_track_step(self.h, B, H, W, _ptr(image), _ptr(hand_side), *[_ptr(o[k]) for k in self._TRACK_ORDER]))
        return o

    def track_step_u8(self, image_u8, hand_side, H=None, W=None, want_kpmap=False):
        """track_step on uint8 frames [B,Hin,Win,3]; tracked steps crop straight from them.  (H, W) default to the frame size,
        the only size the engine accepts here."""
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        hand_side = _f32(hand_side)
        assert img.ndim == 4 and img.shape[3] == 3, "image must be [B,Hin,Win,3] uint8"
        B, Hin, Win, _ = img.shape
        assert hand_side.shape == (B, 2), "hand_side must be [B,2]"
        o = self._track_outputs(B, want_kpmap)
        self._chk(self.lib.hp3d_track_step_u8(self.h, B, Hin, Win, _ptr(img), int(H or Hin), int(W or Win), _ptr(hand_side),
                                              *[_ptr(o[k]) for k in self._TRACK_ORDER]))
        return o

    def track_step_dev(self, B, H, W, image_ptr, hand_side_ptr, crop=0, scale=0, center=0, kpmap=0, coord3d=0, kp_crop=0, kp_hw=0,
                       confidence=0, lost=0, detected=0):
        """Device-pointer variant (ints); stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.lib.hp3d_track_step_dev(self.h, B, H, W, v(image_ptr), v(hand_side_ptr), v(crop), v(scale), v(center), v(kpmap),
                                               v(coord3d), v(kp_crop), v(kp_hw), v(confidence), v(lost), v(detected)))

    # -- NV12 frames (include/hp3d.h "NV12 frames") ------------------------------------
    @staticmethod
    def _nv12_planes(y, uv, W=None):
        """(y, uv) uint8 [B,H,pitch] / [B,H/2,pitch] -> (keepalive, y address, uv address, B, H, W, pitch, frame_stride).  Planes that
        are views of one surface (rows `pitch` bytes apart, both with the same frame stride) are passed as they lie; anything else is
        copied into one [B, 3H/2, pitch] surface.  W defaults to the pitch."""
        y, uv = np.asarray(y), np.asarray(uv)
        assert y.dtype == np.uint8 and uv.dtype == np.uint8 and y.ndim == 3 and uv.ndim == 3, "planes must be uint8 [B,H,pitch] / [B,H/2,pitch]"
        B, H, pitch = y.shape
        assert uv.shape == (B, H // 2, pitch) and H % 2 == 0, "uv must be [B,H/2,pitch] with y's pitch"
        W = pitch if W is None else int(W)
        in_place = (y.strides[1:] == (pitch, 1) and uv.strides[1:] == (pitch, 1) and (B == 1 or (y.strides[0] == uv.strides[0] and y.strides[0] > 0)))
        if not in_place:
            surf = np.concatenate([y, uv], axis=1)
            y, uv = surf[:, :H], surf[:, H:]
        return (y, uv), y.ctypes.data, uv.ctypes.data, B, H, W, pitch, (y.strides[0] if B > 1 else 0)

    def track_step_nv12(self, y, uv, hand_side, W=None, want_kpmap=False):
        """track_step on NV12 frames: y [B,H,pitch], uv [B,H/2,pitch] uint8 (W: the picture's width where pitch > W).  Every output
        equals track_step_u8 on nv12_to_rgb(y, uv) bit for bit; no RGB frame is built."""
        keep, py, puv, B, H, W, pitch, fs = self._nv12_planes(y, uv, W)
        hand_side = _f32(hand_side)
        assert hand_side.shape == (B, 2), "hand_side must be [B,2]"
        o = self._track_outputs(B, want_kpmap)
        self._chk(self.lib.hp3d_track_step_nv12(self.h, B, H, W, C.c_void_p(py), C.c_void_p(puv), pitch, fs, _ptr(hand_side),
                                                *[_ptr(o[k]) for k in self._TRACK_ORDER]))
        return o

    def track_step_nv12_dev(self, B, H, W, y_ptr, uv_ptr, pitch, frame_stride, hand_side_ptr, crop=0, scale=0, center=0, kpmap=0, coord3d=0,
                            kp_crop=0, kp_hw=0, confidence=0, lost=0, detected=0):
        """Device-pointer variant (ints): the surfaces are read in place; stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.lib.hp3d_track_step_nv12_dev(self.h, B, H, W, v(y_ptr), v(uv_ptr), int(pitch), int(frame_stride), v(hand_side_ptr),
                                                    v(crop), v(scale), v(center), v(kpmap), v(coord3d), v(kp_crop), v(kp_hw), v(confidence),
                                                    v(lost), v(detected)))

    def track_hands_step_nv12(self, y, uv, hand_side, max_hands, W=None, want_kpmap=False):
        """track_hands_step on NV12 frames (as track_step_nv12); equals track_hands_step_u8 on the converted frames bit for bit."""
        keep, py, puv, B, H, W, pitch, fs = self._nv12_planes(y, uv, W)
        hand_side = _f32(hand_side)
        K = int(max_hands)
        assert hand_side.shape == (B, K, 2), "hand_side must be [B,max_hands,2]"
        o = self._track_hands_outputs(B, K, want_kpmap)
        self._chk(self.lib.hp3d_track_hands_step_nv12(self.h, B, H, W, C.c_void_p(py), C.c_void_p(puv), pitch, fs, K, _ptr(hand_side),
                                                      *[_ptr(o[k]) for k in self._TRACK_HANDS_ORDER]))
        return o

    def track_hands_step_nv12_dev(self, B, H, W, K, y_ptr, uv_ptr, pitch, frame_stride, hand_side_ptr, crop=0, scale=0, center=0, kpmap=0,
                                  coord3d=0, kp_crop=0, kp_hw=0, confidence=0, lost=0, detected=0, valid=0, area=0, claimed=0):
        """Device-pointer variant (ints): the surfaces are read in place; stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.lib.hp3d_track_hands_step_nv12_dev(self.h, B, H, W, v(y_ptr), v(uv_ptr), int(pitch), int(frame_stride), int(K),
                                                          v(hand_side_ptr), v(crop), v(scale), v(center), v(kpmap), v(coord3d), v(kp_crop),
                                                          v(kp_hw), v(confidence), v(lost), v(detected), v(valid), v(area), v(claimed)))

    def nv12_to_rgb(self, y, uv, W=None):
        """NV12 planes -> uint8 RGB [B,H,W,3] by the rule of include/hp3d.h (option "nv12_matrix")."""
        keep, py, puv, B, H, W, pitch, fs = self._nv12_planes(y, uv, W)
        out = np.empty((B, H, W, 3), np.uint8)
        self._chk(self.lib.hp3d_nv12_to_rgb(self.h, C.c_void_p(py), C.c_void_p(puv), B, H, W, pitch, fs, _ptr(out)))
        return out

    def crop_and_resize_nv12(self, y, uv, center, scale, W=None, K=1, idx=None, crop_size=256):
        """crop_and_resize straight from NV12 frames: center [B*K,2], scale [B*K], K boxes per frame -> [B*K,crop,crop,3]; with idx
        [m] (slot indices) the crops idx[i] only -> [m,crop,crop,3].  = crop_and_resize_u8 / crop_and_resize_idx on nv12_to_rgb."""
        keep, py, puv, B, H, W, pitch, fs = self._nv12_planes(y, uv, W)
        center, scale = _f32(center).reshape(-1, 2), _f32(scale).reshape(-1)
        assert center.shape[0] == B * int(K) and scale.shape[0] == B * int(K), "center / scale must hold B*K boxes"
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = B * int(K) if idx is None else idx.size
        out = np.empty((n, crop_size, crop_size, 3), np.float32)
        self._chk(self.lib.hp3d_crop_and_resize_nv12(self.h, C.c_void_p(py), C.c_void_p(puv), B, H, W, pitch, fs, int(K), _ptr(center),
                                                     _ptr(scale), _ptr(idx), 0 if idx is None else int(idx.size), int(crop_size), _ptr(out)))
        return out

    def downscale_nv12(self, y, uv, f, W=None, idx=None):
        """The detection frame of NV12 frames [B or m,ceil(H/f),ceil(W/f),3] (f = 1: the normalised frame); idx: the frames idx[i]
        only.  = downscale_u8 (f = 1: preprocess_u8 at equal sizes) on nv12_to_rgb, bit for bit."""
        keep, py, puv, B, H, W, pitch, fs = self._nv12_planes(y, uv, W)
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = B if idx is None else idx.size
        out = np.empty((n, -(-H // int(f)), -(-W // int(f)), 3), np.float32)
        self._chk(self.lib.hp3d_downscale_nv12(self.h, C.c_void_p(py), C.c_void_p(puv), B, H, W, pitch, fs, int(f), _ptr(idx),
                                               0 if idx is None else int(idx.size), _ptr(out)))
        return out

    # -- packed 8-bit frames (include/hp3d.h "packed 8-bit frames") ---------------------
    @staticmethod
    def _px_surface(frames, pixel_format):
        """uint8 [B,H,W,pixel_bytes] -> (keepalive, address, B, H, W, pitch, frame_stride, format).  An array whose strides fit the
        layout (last axis 1, pixel stride = pixel_bytes, row stride >= W pixel_bytes, frame stride positive and long enough) -- a padded
        surface, a region of interest of a wider one -- is passed as it lies, with no copy; anything else is copied once."""
        if pixel_format not in FORMATS:
            raise ValueError("pixel_format must be one of %s, got %r" % (', '.join(sorted(FORMATS)), pixel_format))
        fmt, pb, _ = FORMATS[pixel_format]
        a = np.asarray(frames)
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != pb:
            raise ValueError("pixel_format %r wants uint8 frames [B,H,W,%d]" % (pixel_format, pb))
        B, H, W, _ = a.shape
        sb, sr, sp, sc = a.strides
        in_place = sc == 1 and sp == pb and sr >= W * pb and (B == 1 or sb >= sr * (H - 1) + W * pb)
        if not in_place:
            a = np.ascontiguousarray(a)
            sb, sr = a.strides[:2]
        return a, a.ctypes.data, B, H, W, int(sr), (int(sb) if B > 1 else 0), fmt

    def track_step_px(self, frames, pixel_format, hand_side, want_kpmap=False):
        """track_step on packed 8-bit frames: uint8 [B,H,W,pixel_bytes] in `pixel_format` ('rgb', 'bgr', 'rgba', 'bgra', 'argb',
        'abgr'), rows at any pitch (_px_surface).  Every output equals track_step_u8 on the repacked frames bit for bit."""
        keep, p, B, H, W, pitch, fs, fmt = self._px_surface(frames, pixel_format)
        hand_side = _f32(hand_side)
        assert hand_side.shape == (B, 2), "hand_side must be [B,2]"
        o = self._track_outputs(B, want_kpmap)
        self._chk(self.lib.hp3d_track_step_px(self.h, B, H, W, C.c_void_p(p), pitch, fs, fmt, _ptr(hand_side),
                                              *[_ptr(o[k]) for k in self._TRACK_ORDER]))
        return o

    def track_step_px_dev(self, B, H, W, px_ptr, pitch, frame_stride, pixel_format, hand_side_ptr, crop=0, scale=0, center=0, kpmap=0,
                          coord3d=0, kp_crop=0, kp_hw=0, confidence=0, lost=0, detected=0):
        """Device-pointer variant (ints): the surface is read in place; stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.lib.hp3d_track_step_px_dev(self.h, B, H, W, v(px_ptr), int(pitch), int(frame_stride), FORMATS[pixel_format][0],
                                                  v(hand_side_ptr), v(crop), v(scale), v(center), v(kpmap), v(coord3d), v(kp_crop), v(kp_hw),
                                                  v(confidence), v(lost), v(detected)))

    def track_hands_step_px(self, frames, pixel_format, hand_side, max_hands, want_kpmap=False):
        """track_hands_step on packed 8-bit frames (as track_step_px); equals track_hands_step_u8 on the repacked frames bit for bit."""
        keep, p, B, H, W, pitch, fs, fmt = self._px_surface(frames, pixel_format)
        hand_side = _f32(hand_side)
        K = int(max_hands)
        assert hand_side.shape == (B, K, 2), "hand_side must be [B,max_hands,2]"
        o = self._track_hands_outputs(B, K, want_kpmap)
        self._chk(self.lib.hp3d_track_hands_step_px(self.h, B, H, W, C.c_void_p(p), pitch, fs, fmt, K, _ptr(hand_side),
                                                    *[_ptr(o[k]) for k in self._TRACK_HANDS_ORDER]))
        return o

    def track_hands_step_px_dev(self, B, H, W, K, px_ptr, pitch, frame_stride, pixel_format, hand_side_ptr, crop=0, scale=0, center=0,
                                kpmap=0, coord3d=0, kp_crop=0, kp_hw=0, confidence=0, lost=0, detected=0, valid=0, area=0, claimed=0):
        """Device-pointer variant (ints): the surface is read in place; stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.lib.hp3d_track_hands_step_px_dev(self.h, B, H, W, v(px_ptr), int(pitch), int(frame_stride), FORMATS[pixel_format][0],
                                                        int(K), v(hand_side_ptr), v(crop), v(scale), v(center), v(kpmap), v(coord3d),
                                                        v(kp_crop), v(kp_hw), v(confidence), v(lost), v(detected), v(valid), v(area),
                                                        v(claimed)))

    def px_to_rgb(self, frames, pixel_format):
        """Packed 8-bit frames -> uint8 RGB [B,H,W,3] (= utils.pixels.to_rgb)."""
        keep, p, B, H, W, pitch, fs, fmt = self._px_surface(frames, pixel_format)
        out = np.empty((B, H, W, 3), np.uint8)
        self._chk(self.lib.hp3d_px_to_rgb(self.h, C.c_void_p(p), B, H, W, pitch, fs, fmt, _ptr(out)))
        return out

    def crop_and_resize_px(self, frames, pixel_format, center, scale, K=1, idx=None, crop_size=256):
        """crop_and_resize straight from packed 8-bit frames: center [B*K,2], scale [B*K], K boxes per frame -> [B*K,crop,crop,3]; with
        idx [m] (slot indices) the crops idx[i] only -> [m,crop,crop,3].  = crop_and_resize_u8 / crop_and_resize_idx on px_to_rgb."""
        keep, p, B, H, W, pitch, fs, fmt = self._px_surface(frames, pixel_format)
        center, scale = _f32(center).reshape(-1, 2), _f32(scale).reshape(-1)
        assert center.shape[0] == B * int(K) and scale.shape[0] == B * int(K), "center / scale must hold B*K boxes"
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = B * int(K) if idx is None else idx.size
        out = np.empty((n, crop_size, crop_size, 3), np.float32)
        self._chk(self.lib.hp3d_crop_and_resize_px(self.h, C.c_void_p(p), B, H, W, pitch, fs, fmt, int(K), _ptr(center), _ptr(scale),
                                                   _ptr(idx), 0 if idx is None else int(idx.size), int(crop_size), _ptr(out)))
        return out

    def downscale_px(self, frames, pixel_format, f, idx=None):
        """The detection frame of packed 8-bit frames [B or m,ceil(H/f),ceil(W/f),3] (f = 1: the normalised frame); idx: the frames
        idx[i] only.  = downscale_u8 (f = 1: preprocess_u8 at equal sizes) on px_to_rgb, bit for bit."""
        keep, p, B, H, W, pitch, fs, fmt = self._px_surface(frames, pixel_format)
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = B if idx is None else idx.size
        out = np.empty((n, -(-H // int(f)), -(-W // int(f)), 3), np.float32)
        self._chk(self.lib.hp3d_downscale_px(self.h, C.c_void_p(p), B, H, W, pitch, fs, fmt, int(f), _ptr(idx),
                                             0 if idx is None else int(idx.size), _ptr(out)))
        return out

    # -- a batch of separate surfaces, formats mixed (include/hp3d.h) -------------------
    @staticmethod
    def surface_records(records):
        """[(data address, chroma address or 0, pitch, format, height, width)] -> the hp3d_surface array of the C ABI.  `format` is a
        name ('rgb' ... 'abgr', 'nv12') or the ABI's number."""
        arr = (Surface * max(len(records), 1))()
        for r, (data, chroma, pitch, fmt, height, width) in zip(arr, records):
            r.data, r.chroma = int(data) or None, int(chroma) or None
            r.pitch, r.height, r.width = int(pitch), int(height), int(width)
            r.format = SURF_NV12 if fmt == 'nv12' else FORMATS[fmt][0] if fmt in FORMATS else int(fmt)
        return arr

    @classmethod
    def _surfaces(cls, surfaces, formats):
        """B surfaces and their B format names -> (keepalive, hp3d_surface array, B, H, W).  A packed surface is uint8 [H,W,pixel_bytes],
        an NV12 one a pair (y [H,W], uv [H/2,W]) of uint8 planes under the name 'nv12'; the pitch comes from the array's strides, so a
        padded surface or a region of interest of a wider one is passed as it lies (anything else is copied once)."""
        surfaces, formats = list(surfaces), list(formats)
        if not surfaces or len(surfaces) != len(formats):
            raise ValueError("%d surfaces, %d formats: need one format per surface and at least one surface" % (len(surfaces), len(formats)))
        keep, recs, H, W = [], [], None, None
        for i, (s, f) in enumerate(zip(surfaces, formats)):
            if f == 'nv12':
                if not isinstance(s, (tuple, list)) or len(s) != 2:
                    raise ValueError("surface %d: format 'nv12' wants a pair (y [H,W], uv [H/2,W]) of uint8 planes" % i)
                y, uv = np.asarray(s[0]), np.asarray(s[1])
                if y.dtype != np.uint8 or uv.dtype != np.uint8 or y.ndim != 2 or uv.shape != (y.shape[0] // 2, y.shape[1]) or y.shape[0] % 2:
                    raise ValueError("surface %d: format 'nv12' wants a pair (y [H,W], uv [H/2,W]) of uint8 planes" % i)
                if not (y.strides[1] == 1 and uv.strides == y.strides and y.strides[0] >= y.shape[1]):
                    surf = np.concatenate([y, uv], axis=0)
                    y, uv = surf[:y.shape[0]], surf[y.shape[0]:]
                keep.append((y, uv))
                recs.append((y.ctypes.data, uv.ctypes.data, y.strides[0], 'nv12') + y.shape)
            else:
                if f not in FORMATS:
                    raise ValueError("surface %d: format must be 'nv12' or one of %s, got %r" % (i, ', '.join(sorted(FORMATS)), f))
                pb = FORMATS[f][1]
                if isinstance(s, tuple):
                    raise ValueError("surface %d: format %r names a packed frame; (y, uv) is a pair of NV12 planes" % (i, f))
                a = np.asarray(s)
                if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != pb:
                    raise ValueError("surface %d: format %r wants a uint8 frame [H,W,%d]" % (i, f, pb))
                if not (a.strides[2] == 1 and a.strides[1] == pb and a.strides[0] >= a.shape[1] * pb):
                    a = np.ascontiguousarray(a)
                keep.append(a)
                recs.append((a.ctypes.data, 0, a.strides[0], f) + a.shape[:2])
            if H is None:
                H, W = recs[-1][4:]
        return keep, cls.surface_records(recs), len(recs), int(H), int(W)

    def track_step_surf(self, surfaces, formats, hand_side, want_kpmap=False):
        """track_step on B separate surfaces in B formats (_surfaces).  Every output equals track_step_u8 on the stack of the surfaces'
        RGB frames (utils.pixels.surfaces_to_rgb) bit for bit."""
        keep, arr, B, H, W = self._surfaces(surfaces, formats)
        hand_side = _f32(hand_side)
        assert hand_side.shape == (B, 2), "hand_side must be [B,2]"
        o = self._track_outputs(B, want_kpmap)
        self._chk(self.lib.hp3d_track_step_surf(self.h, B, H, W, C.addressof(arr), _ptr(hand_side), *[_ptr(o[k]) for k in self._TRACK_ORDER]))
        return o

    def track_step_surf_dev(self, B, H, W, records, hand_side_ptr, crop=0, scale=0, center=0, kpmap=0, coord3d=0, kp_crop=0, kp_hw=0,
                            confidence=0, lost=0, detected=0):
        """Device-pointer variant (ints).  records: B tuples (data address, chroma address or 0, pitch, format name) of device surfaces,
        read in place; stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        arr = self.surface_records([tuple(r) + (H, W) for r in records])
        self._chk(self.lib.hp3d_track_step_surf_dev(self.h, B, H, W, C.addressof(arr), v(hand_side_ptr), v(crop), v(scale), v(center), v(kpmap),
                                                    v(coord3d), v(kp_crop), v(kp_hw), v(confidence), v(lost), v(detected)))

    def track_hands_step_surf(self, surfaces, formats, hand_side, max_hands, want_kpmap=False):
        """track_hands_step on B separate surfaces (as track_step_surf); equals track_hands_step_u8 on the stacked RGB frames bit for bit."""
        keep, arr, B, H, W = self._surfaces(surfaces, formats)
        hand_side = _f32(hand_side)
        K = int(max_hands)
        assert hand_side.shape == (B, K, 2), "hand_side must be [B,max_hands,2]"
        o = self._track_hands_outputs(B, K, want_kpmap)
        self._chk(self.lib.hp3d_track_hands_step_surf(self.h, B, H, W, C.addressof(arr), K, _ptr(hand_side),
                                                      *[_ptr(o[k]) for k in self._TRACK_HANDS_ORDER]))
        return o

    def track_hands_step_surf_dev(self, B, H, W, K, records, hand_side_ptr, crop=0, scale=0, center=0, kpmap=0, coord3d=0, kp_crop=0, kp_hw=0,
                                  confidence=0, lost=0, detected=0, valid=0, area=0, claimed=0):
        """Device-pointer variant (ints; records as for track_step_surf_dev); stream-ordered, call sync() before reading."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        arr = self.surface_records([tuple(r) + (H, W) for r in records])
        self._chk(self.lib.hp3d_track_hands_step_surf_dev(self.h, B, H, W, C.addressof(arr), int(K), v(hand_side_ptr), v(crop), v(scale),
                                                          v(center), v(kpmap), v(coord3d), v(kp_crop), v(kp_hw), v(confidence), v(lost),
                                                          v(detected), v(valid), v(area), v(claimed)))

    def surf_to_rgb(self, surfaces, formats):
        """B surfaces -> uint8 RGB [B,H,W,3] (= utils.pixels.surfaces_to_rgb under option "nv12_matrix")."""
        keep, arr, B, H, W = self._surfaces(surfaces, formats)
        out = np.empty((B, H, W, 3), np.uint8)
        self._chk(self.lib.hp3d_surf_to_rgb(self.h, C.addressof(arr), B, H, W, _ptr(out)))
        return out

    def crop_and_resize_surf(self, surfaces, formats, center, scale, K=1, idx=None, crop_size=256):
        """crop_and_resize straight from B surfaces: center [B*K,2], scale [B*K], K boxes per frame -> [B*K,crop,crop,3]; with idx [m]
        (slot indices) the crops idx[i] only.  = crop_and_resize_u8 / crop_and_resize_idx on surf_to_rgb."""
        keep, arr, B, H, W = self._surfaces(surfaces, formats)
        center, scale = _f32(center).reshape(-1, 2), _f32(scale).reshape(-1)
        assert center.shape[0] == B * int(K) and scale.shape[0] == B * int(K), "center / scale must hold B*K boxes"
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = B * int(K) if idx is None else idx.size
        out = np.empty((n, crop_size, crop_size, 3), np.float32)
        self._chk(self.lib.hp3d_crop_and_resize_surf(self.h, C.addressof(arr), B, H, W, int(K), _ptr(center), _ptr(scale), _ptr(idx),
                                                     0 if idx is None else int(idx.size), int(crop_size), _ptr(out)))
        return out

    def downscale_surf(self, surfaces, formats, f, idx=None):
        """The detection frame of B surfaces [B or m,ceil(H/f),ceil(W/f),3] (f = 1: the normalised frame); idx: the frames idx[i] only.
        = downscale_u8 (f = 1: preprocess_u8 at equal sizes) on surf_to_rgb, bit for bit."""
        keep, arr, B, H, W = self._surfaces(surfaces, formats)
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = B if idx is None else idx.size
        out = np.empty((n, -(-H // int(f)), -(-W // int(f)), 3), np.float32)
        self._chk(self.lib.hp3d_downscale_surf(self.h, C.addressof(arr), B, H, W, int(f), _ptr(idx), 0 if idx is None else int(idx.size),
                                               _ptr(out)))
        return out

    def track_box(self, keypoint_hw, H, W, score32=None, margin=None):
        """The next crop box from 21 image-space keypoints [B,21,2] (row, col): (center [B,2], scale [B], confidence [B], lost [B]).
        margin=None uses option "track_margin"; margin=1 is the dataset readers' hand_crop rule bit for bit."""
        kp = np.ascontiguousarray(keypoint_hw, dtype=np.float64)
        assert kp.ndim == 3 and kp.shape[1:] == (21, 2), "keypoint_hw must be [B,21,2]"
        B = kp.shape[0]
        sm = None if score32 is None else _f32(score32)
        assert sm is None or sm.shape == (B, 32, 32, 21), "score32 must be [B,32,32,21]"
        center, scale = np.empty((B, 2), np.float32), np.empty((B,), np.float32)
        conf, lost = np.empty((B,), np.float32), np.empty((B,), np.int32)
        assert margin is None or margin > 0, "margin must be positive"
        self._chk(self.lib.hp3d_track_box(self.h, B, int(H), int(W), _ptr(kp), _ptr(sm), 0.0 if margin is None else float(margin),
                                          _ptr(center), _ptr(scale), _ptr(conf), _ptr(lost)))
        return center, scale, conf, lost

    def crop_and_resize_u8(self, image_u8, center, scale, crop_size=256):
        """crop_and_resize straight from uint8 frames [B,H,W,3] (= preprocess_u8 at equal sizes -> crop_and_resize, bit for bit)."""
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        center, scale = _f32(center), _f32(scale).reshape(-1)
        assert img.ndim == 4 and img.shape[3] == 3, "image must be [B,H,W,3] uint8"
        B, H, W, _ = img.shape
        out = np.empty((B, crop_size, crop_size, 3), np.float32)
        self._chk(self.lib.hp3d_crop_and_resize_u8(self.h, _ptr(img), B, H, W, _ptr(center), _ptr(scale), crop_size, _ptr(out)))
        return out

    # -- detection on a reduced frame (include/hp3d.h): the per-op forms ----------------
    def crop_and_resize_idx(self, image, center, scale, idx, K, crop_size=256):
        """Crop i = box idx[i] of center [B*K,2] / scale [B*K], cut from image idx[i] // K (option "hands_compact").
        image [B,H,W,3] float32 or uint8 (then normalised tap by tap as preprocess_u8 does) -> [m,crop_size,crop_size,3]."""
        u8 = np.asarray(image).dtype == np.uint8
        image = np.ascontiguousarray(image, dtype=np.uint8 if u8 else np.float32)
        B, H, W, _ = image.shape
        center, scale = _f32(center), _f32(scale)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.empty((idx.size, crop_size, crop_size, 3), np.float32)
        self._chk(self.lib.hp3d_crop_and_resize_idx(self.h, None if u8 else _ptr(image), _ptr(image) if u8 else None, B, H, W, int(K),
                                                    _ptr(center), _ptr(scale), _ptr(idx), int(idx.size), int(crop_size), _ptr(out)))
        return out

    def slot_scatter(self, dense, pos, skew_words=0, sentinel=-7.0):
        """dense [m,...] (any 4-byte dtype) -> [ns,...] with out[s] = dense[pos[s]], 0 where pos[s] = -1 (option "hands_compact").
        Returns (out, tail): tail = the 4 words behind the last slot, which were `sentinel` before the launch."""
        dense = np.ascontiguousarray(dense)
        assert dense.dtype.itemsize == 4
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        m, ns = dense.shape[0], pos.size
        words = int(np.prod(dense.shape[1:]))
        buf = np.full(ns * words + 4, sentinel, np.float32)
        self._chk(self.lib.hp3d_slot_scatter(self.h, _ptr(dense.view(np.float32)) if m else None, _ptr(pos), ns, m, words, int(skew_words),
                                             _ptr(buf)))
        return buf[:ns * words].view(dense.dtype).reshape((ns,) + dense.shape[1:]), buf[ns * words:]

    def downscale(self, image, f):
        """The detection frame of float32 frames [B,H,W,3]: the f x f area mean [B,ceil(H/f),ceil(W/f),3] (clipped windows)."""
        image = _f32(image)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        out = np.empty((B, -(-H // int(f)), -(-W // int(f)), 3), np.float32)
        self._chk(self.lib.hp3d_downscale(self.h, _ptr(image), B, H, W, int(f), _ptr(out)))
        return out

    def downscale_u8(self, image_u8, f):
        """downscale of uint8 frames [B,H,W,3], normalised (mean / 255 - 0.5) from the exact integer window sums."""
        img = np.ascontiguousarray(image_u8, dtype=np.uint8)
        assert img.ndim == 4 and img.shape[3] == 3, "image must be [B,H,W,3] uint8"
        B, H, W, _ = img.shape
        out = np.empty((B, -(-H // int(f)), -(-W // int(f)), 3), np.float32)
        self._chk(self.lib.hp3d_downscale_u8(self.h, _ptr(img), B, H, W, int(f), _ptr(out)))
        return out

    def gather_frames(self, image, idx, f=1):
        """The frames idx (strictly ascending) of image [B,H,W,3], as a detect step of option "track_partial_detect" hands them to
        HandSegNet -> [m,ceil(H/f),ceil(W/f),3] float32: float32 frames copied (f = 1) or downscaled; uint8 frames
        normalised (x / 255 - 0.5, f = 1) or downscaled as downscale_u8 does."""
        u8 = np.asarray(image).dtype == np.uint8
        image = np.ascontiguousarray(image, dtype=np.uint8 if u8 else np.float32)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        out = np.empty((idx.size, -(-H // max(int(f), 1)), -(-W // max(int(f), 1)), 3), np.float32)
        self._chk(self.lib.hp3d_gather_frames(self.h, None if u8 else _ptr(image), _ptr(image) if u8 else None, B, H, W, int(f),
                                              _ptr(idx), int(idx.size), _ptr(out)))
        return out

    # -- the multi-hand tracker's partial detection (option "track_hands_partial_detect"): the per-op forms ----
    def track_hands_partial_index(self, valid, lost):
        """valid / lost int32 [nb,K] -> (idx [m], pos [nb], m): the frames that have a valid slot lost or no valid slot, ascending, and
        every frame's index among them (-1: not one of them), as a partial detect step builds them on the device."""
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        lost = np.ascontiguousarray(lost, dtype=np.int32)
        assert valid.ndim == 2 and lost.shape == valid.shape, "valid and lost must be [nb,K]"
        nb, K = valid.shape
        idx, pos = np.empty((nb,), np.int32), np.empty((nb,), np.int32)
        m = C.c_int32(-1)
        self._chk(self.lib.hp3d_track_hands_partial_index(self.h, nb, K, _ptr(valid), _ptr(lost), _ptr(idx), _ptr(pos), C.byref(m)))
        assert np.all(idx[m.value:] == -1)
        return idx[:m.value].copy(), pos, int(m.value)

    def track_hands_select_pos(self, pos, keep, det, box_center, box_scale, valid):
        """A partial detect step's per-slot choice: pos [nb], keep [nb,K], det = dict of the growth's dense center [m,K,2], scale,
        valid, area, claimed [m,K] (masks_from_scoremap(keep=...)'s), the state's box_center [nb,K,2], box_scale [nb,K], valid [nb,K]
        -> dict of center, scale, valid, detected, area, claimed per slot."""
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        keep = np.ascontiguousarray(keep, dtype=np.int32)
        nb, K = keep.shape
        assert pos.shape == (nb,)
        dc, ds = _f32(det['center']).copy(), _f32(det['scale']).copy()
        dv, da, dk = [np.ascontiguousarray(det[k], dtype=np.int32) for k in ('valid', 'area', 'claimed')]
        m = ds.shape[0]
        assert dc.shape == (m, K, 2) and ds.shape == dv.shape == da.shape == dk.shape == (m, K)
        o = {'center': _f32(box_center).copy(), 'scale': _f32(box_scale).copy(), 'valid': np.array(valid, dtype=np.int32, order='C'),
             'detected': np.empty((nb, K), np.int32), 'area': np.empty((nb, K), np.int32), 'claimed': np.empty((nb, K), np.int32)}
        assert o['center'].shape == (nb, K, 2) and o['scale'].shape == (nb, K) and o['valid'].shape == (nb, K)
        self._chk(self.lib.hp3d_track_hands_select_pos(self.h, nb, K, m, _ptr(pos), _ptr(keep), _ptr(dc), _ptr(ds), _ptr(dv), _ptr(da),
                                                       _ptr(dk), *[_ptr(o[k]) for k in ('center', 'scale', 'valid', 'detected', 'area',
                                                                                        'claimed')]))
        return o

    def boxes_to_frame(self, center_d, crop_size_d, f):
        """Detection-frame boxes (center_d [...,2], crop_size_d [...]) in frame coordinates: (center, crop_size, scale)."""
        cd, sd = _f32(center_d), _f32(crop_size_d)
        assert cd.shape == sd.shape + (2,), "center_d must be [...,2], crop_size_d [...]"
        center, size, scale = np.empty_like(cd), np.empty_like(sd), np.empty_like(sd)
        self._chk(self.lib.hp3d_boxes_to_frame(self.h, sd.size, int(f), _ptr(cd), _ptr(sd), _ptr(center), _ptr(size), _ptr(scale)))
        return center, size, scale

    def boxes_to_detect(self, center, scale, f):
        """Frame boxes (center [...,2], scale [...]) in detection-frame coordinates: (center_d, scale_d)."""
        c, s = _f32(center), _f32(scale)
        assert c.shape == s.shape + (2,), "center must be [...,2], scale [...]"
        cd, sd = np.empty_like(c), np.empty_like(s)
        self._chk(self.lib.hp3d_boxes_to_detect(self.h, s.size, int(f), _ptr(c), _ptr(s), _ptr(cd), _ptr(sd)))
        return cd, sd

    def infer_2d(self, image):
        image = _f32(image)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        kp = np.empty((B, 256, 256, 21), np.float32)
        crop = np.empty((B, 256, 256, 3), np.float32)
        scale = np.empty((B, 1), np.float32)
        center = np.empty((B, 2), np.float32)
        self._chk(self.lib.hp3d_infer_2d(self.h, B, H, W, _ptr(image), _ptr(kp), _ptr(crop), _ptr(scale), _ptr(center)))
        return kp, crop, scale, center

    def infer_2d_keypoints(self, image, want_scoremap=False):
        """inference2d + detect_keypoints + trafo_coords on the device (eval2d.py:58,93-94): returns
        (kp_crop int32 [B,21,2], kp_hw float64 [B,21,2], scale_crop, center[, keypoints_scoremap])."""
        image = _f32(image)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        kp = np.empty((B, 256, 256, 21), np.float32) if want_scoremap else None
        scale = np.empty((B, 1), np.float32)
        center = np.empty((B, 2), np.float32)
        kpc = np.empty((B, 21, 2), np.int32)
        kph = np.empty((B, 21, 2), np.float64)
        self._chk(self.lib.hp3d_infer_2d_kp(self.h, B, H, W, _ptr(image), _ptr(kp), None, _ptr(scale), _ptr(center),
                                            _ptr(kpc), _ptr(kph)))
        return (kpc, kph, scale, center, kp) if want_scoremap else (kpc, kph, scale, center)

    def detect_keypoints(self, scoremap, out_hw=(256, 256)):
        """detect_keypoints(resize_images(scoremap, out_hw)) per image: [B,h,w,C] -> int32 [B,C,2]."""
        x = _f32(scoremap)
        B, h, w, Cc = x.shape
        out = np.empty((B, Cc, 2), np.int32)
        self._chk(self.lib.hp3d_detect_keypoints(self.h, _ptr(x), B, h, w, Cc, int(out_hw[0]), int(out_hw[1]), _ptr(out)))
        return out

    def handsegnet(self, image, want_small=False):
        image = _f32(image)
        assert image.ndim == 4 and image.shape[3] == 3, "image must be [B,H,W,3]"
        B, H, W, _ = image.shape
        large = np.empty((B, H, W, 2), np.float32)
        small = np.empty((B, H // 8, W // 8, 2), np.float32) if want_small else None
        self._chk(self.lib.hp3d_handsegnet(self.h, B, H, W, _ptr(image), _ptr(large), _ptr(small)))
        return (large, small) if want_small else large

    def posenet2d(self, image_crop):
        image_crop = _f32(image_crop)
        assert image_crop.ndim == 4 and image_crop.shape[3] == 3, "image_crop must be [B,H,W,3]"
        B, H, W, _ = image_crop.shape
        outs = [np.empty((B, H // 8, W // 8, 21), np.float32) for _ in range(3)]
        self._chk(self.lib.hp3d_posenet2d(self.h, B, H, W, _ptr(image_crop), *[_ptr(x) for x in outs]))
        return outs

    def poseprior(self, variant, scoremap256, hand_side):
        assert variant in VARIANTS, "Unknown variant."
        sm, hs = _f32(scoremap256), _f32(hand_side)
        assert sm.ndim == 4 and sm.shape[1:] == (256, 256, 21), "scoremap must be [B,256,256,21]"
        B = sm.shape[0]
        rel = np.empty((B, 21, 3), np.float32)
        c3d = np.empty((B, 21, 3), np.float32)
        R = np.empty((B, 3, 3), np.float32)
        self._chk(self.lib.hp3d_poseprior(self.h, B, VARIANTS[variant], _ptr(sm), _ptr(hs), _ptr(rel), _ptr(c3d), _ptr(R)))
        return rel, c3d, (R if variant == 'proposed' else None)

    def pose3d(self, scoremap32, hand_side):
        sm, hs = _f32(scoremap32), _f32(hand_side)
        B = sm.shape[0]
        assert sm.shape[1:] == (32, 32, 21)
        rel = np.empty((B, 21, 3), np.float32)
        can = np.empty((B, 21, 3), np.float32)
        R = np.empty((B, 3, 3), np.float32)
        self._chk(self.lib.hp3d_pose3d(self.h, B, _ptr(sm), _ptr(hs), _ptr(rel), _ptr(can), _ptr(R)))
        return rel, can, R

    # -- per-op ------------------------------------------------------------------------------
    def conv2d(self, x, w, b, stride=1, act=True, pool=False):
        x, w, b = _f32(x), _f32(w), _f32(b)
        B, H, W, Cin = x.shape
        k, _, _, Cout = w.shape
        Ho, Wo = -(-H // stride), -(-W // stride)
        if pool:
            Ho, Wo = Ho // 2, Wo // 2
        out = np.empty((B, Ho, Wo, Cout), np.float32)
        self._chk(self.lib.hp3d_conv2d(self.h, _ptr(x), B, H, W, Cin, _ptr(w), _ptr(b), k, stride, Cout, int(act),
                                       int(pool), _ptr(out)))
        return out

    def conv2d_f16(self, x, w, b, stride=1, act=True, pool=False, out_f32=False):
        """One layer of a half-precision trunk (hp3d_conv2d_f16): float32 in and out, half operands and (unless out_f32) a half result."""
        x, w, b = _f32(x), _f32(w), _f32(b)
        B, H, W, Cin = x.shape
        k, _, _, Cout = w.shape
        Ho, Wo = -(-H // stride), -(-W // stride)
        if pool:
            Ho, Wo = Ho // 2, Wo // 2
        out = np.empty((B, Ho, Wo, Cout), np.float32)
        self._chk(self.lib.hp3d_conv2d_f16(self.h, _ptr(x), B, H, W, Cin, _ptr(w), _ptr(b), k, stride, Cout, int(act),
                                           int(pool), int(out_f32), _ptr(out)))
        return out

    def first_block_f16(self, image, w1, b1, w2, b2):
        """conv1_1 + conv1_2 + 2x2 max-pool of a half-precision trunk (hp3d_first_block_f16): image [B,H,W,3] -> [B,H/2,W/2,64]."""
        image, w1, b1, w2, b2 = _f32(image), _f32(w1), _f32(b1), _f32(w2), _f32(b2)
        B, H, W, c3 = image.shape
        assert c3 == 3 and w1.shape == (3, 3, 3, 64) and w2.shape == (3, 3, 64, 64) and b1.shape == (64,) and b2.shape == (64,)
        out = np.empty((B, H // 2, W // 2, 64), np.float32)
        self._chk(self.lib.hp3d_first_block_f16(self.h, _ptr(image), B, H, W, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(out)))
        return out

    def maxpool2(self, x):
        x = _f32(x)
        B, H, W, Cc = x.shape
        out = np.empty((B, H // 2, W // 2, Cc), np.float32)
        self._chk(self.lib.hp3d_maxpool2(self.h, _ptr(x), B, H, W, Cc, _ptr(out)))
        return out

    def avgpool8(self, x):
        x = _f32(x)
        B, H, W, Cc = x.shape
        out = np.empty((B, H // 8, W // 8, Cc), np.float32)
        self._chk(self.lib.hp3d_avgpool8(self.h, _ptr(x), B, H, W, Cc, _ptr(out)))
        return out

    def resize_bilinear(self, x, oh, ow):
        x = _f32(x)
        B, H, W, Cc = x.shape
        out = np.empty((B, oh, ow, Cc), np.float32)
        self._chk(self.lib.hp3d_resize_bilinear(self.h, _ptr(x), B, H, W, Cc, oh, ow, _ptr(out)))
        return out

    def crop_and_resize(self, image, center, scale, crop_size=256):
        image, center, scale = _f32(image), _f32(center), _f32(scale).reshape(-1)
        B, H, W, Cc = image.shape
        out = np.empty((B, crop_size, crop_size, Cc), np.float32)
        self._chk(self.lib.hp3d_crop_and_resize(self.h, _ptr(image), B, H, W, Cc, _ptr(center), _ptr(scale), crop_size,
                                                _ptr(out)))
        return out

    def mask_from_scoremap(self, scoremap):
        sm = _f32(scoremap)
        B, H, W, c2 = sm.shape
        assert c2 == 2
        mask = np.empty((B, H, W), np.float32)
        center = np.empty((B, 2), np.float32)
        size = np.empty((B, 1), np.float32)
        scale = np.empty((B, 1), np.float32)
        seed = np.empty((B, 2), np.int32)
        self._chk(self.lib.hp3d_mask_from_scoremap(self.h, _ptr(sm), B, H, W, _ptr(mask), _ptr(center), _ptr(size),
                                                   _ptr(scale), _ptr(seed)))
        return mask, center, size, scale, seed

    def fc(self, x, w, b, act=False):
        x, w, b = _f32(x), _f32(w), _f32(b)
        B, Cin = x.shape
        Cout = w.shape[1]
        out = np.empty((B, Cout), np.float32)
        self._chk(self.lib.hp3d_fc(self.h, _ptr(x), B, Cin, _ptr(w), _ptr(b), Cout, int(act), _ptr(out)))
        return out

    def argmax2d(self, x):
        x = _f32(x)
        B, H, W, Cc = x.shape
        out = np.empty((B, Cc, 2), np.int32)
        self._chk(self.lib.hp3d_argmax2d(self.h, _ptr(x), B, H, W, Cc, _ptr(out)))
        return out

    # -- measurement -------------------------------------------------------------------------
    def set_profiling(self, on):
        self._chk(self.lib.hp3d_set_profiling(self.h, int(on)))

    def counter(self, name):
        v = C.c_longlong()
        self._chk(self.lib.hp3d_get_counter(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def get_timing(self):
        """{stage: GPU ms} over the profiled launches (hp3d_get_timing; stages: TIMING_STAGES)."""
        buf = (C.c_float * len(TIMING_STAGES))()
        self._chk(self.lib.hp3d_get_timing(self.h, buf, len(TIMING_STAGES)))
        return dict(zip(TIMING_STAGES, [float(v) for v in buf]))

    # -- multi-GPU: native RCCL on the engine stream -------------------------------
    def comm_unique_id(self):
        """128-byte RCCL id (create on ONE rank, hand to the others through the launcher's side channel)."""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        self._chk(self.lib.hp3d_comm_unique_id(buf))
        return bytes(buf.raw)

    def comm_init(self, rank, world, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        self._chk(self.lib.hp3d_comm_init(self.h, int(rank), int(world), C.c_char_p(bytes(unique_id))))

    def bcast_weights(self, root=0):
        self._chk(self.lib.hp3d_bcast_weights(self.h, int(root)))

    def allgather(self, local, world):
        """all-gather of equal-sized float32 arrays: [n, ...] per rank -> [world * n, ...]."""
        a = _f32(local)
        out = np.empty((int(world) * a.shape[0],) + a.shape[1:], np.float32)
        self._chk(self.lib.hp3d_allgather(self.h, _ptr(a), a.size, _ptr(out)))
        return out

    def allgather_dev(self, dev_buf, count, world):
        """all-gather straight from a device buffer of `count` floats per rank -> float32 [world * count] on the host."""
        out = np.empty(int(world) * int(count), np.float32)
        self._chk(self.lib.hp3d_allgather_dev(self.h, C.c_void_p(int(dev_buf)), int(count), _ptr(out)))
        return out

    def comm_destroy(self):
        self._chk(self.lib.hp3d_comm_destroy(self.h))

    # -- device / pinned host memory through the C ABI (no torch) ---------------------------------------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.hp3d_dev_alloc(self.h, int(nbytes), C.byref(p)))
        return DevBuf(self, p.value, int(nbytes))

    def to_device(self, array):
        """Copy a NumPy array into a fresh device buffer (blocking)."""
        a = np.ascontiguousarray(array)
        buf = self.dev_alloc(a.nbytes)
        self._chk(self.lib.hp3d_memcpy(self.h, C.c_void_p(buf.ptr), _ptr(a), a.nbytes, 0))
        return buf

    def to_host(self, buf, shape, dtype=np.float32, offset_bytes=0):
        out = np.empty(shape, dtype)
        self._chk(self.lib.hp3d_memcpy(self.h, _ptr(out), C.c_void_p(int(buf) + int(offset_bytes)), out.nbytes, 1))
        return out

    def pinned_empty(self, shape, dtype=np.float32):
        """NumPy array over page-locked host memory (for hp3d_upload_async).  The memory belongs to the engine: it is released
        by close() (after pending uploads have finished), so the array must not be used past that point."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self.lib.hp3d_host_alloc(self.h, n, C.byref(p)))
        arr = np.frombuffer((C.c_char * n).from_address(p.value), dtype=dtype).reshape(shape)
        self._pinned.append(p.value)
        return arr

    def upload_async(self, buf, pinned_array):
        self._chk(self.lib.hp3d_upload_async(self.h, C.c_void_p(int(buf)), _ptr(pinned_array), pinned_array.nbytes))

    def wait_upload(self):
        self._chk(self.lib.hp3d_wait_upload(self.h))

    def profile(self):
        """[(layer, kernel, ms, flops, bytes)] of the last whole-path call."""
        n = self.lib.hp3d_prof_count(self.h)
        rows = []
        name, kern = C.create_string_buffer(96), C.create_string_buffer(96)
        ms, fl, by = C.c_float(), C.c_double(), C.c_double()
        for i in range(n):
            self._chk(self.lib.hp3d_prof_get(self.h, i, name, 96, kern, 96, C.byref(ms), C.byref(fl), C.byref(by)))
            rows.append((name.value.decode(), kern.value.decode(), ms.value, fl.value, by.value))
        return rows
