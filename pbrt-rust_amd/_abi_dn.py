"""ctypes mirror of include/mi355dn.h (libmi355dn.so: the a-trous denoiser over two half films and the feature buffers). Kept apart from
_abi.py, which mirrors include/mi355pt.h alone."""
import ctypes as C
from ._abi import VP, f32, u32
from ._abi_aov import PtAOVBuffers


class PtDenoiseParams(C.Structure):
    _fields_ = [("iterations", u32), ("sigma_l", f32), ("sigma_z", f32), ("sigma_n", f32), ("albedo_floor", f32), ("scale", f32)]


# Every symbol include/mi355dn.h declares, with its signature (restype, argtypes). The buffers are void*: host arrays or device pointers, by the last argument.
ENTRY_POINTS = {
    "pt_denoise_default_params": (None, [C.POINTER(PtDenoiseParams)]),
    "pt_denoise": (C.c_int, [VP, C.POINTER(PtDenoiseParams), VP, VP, C.POINTER(PtAOVBuffers), u32, u32, VP, C.c_int]),
}
