"""ctypes mirror of include/mi355aov.h (libmi355aov.so: the feature buffers for denoising -- albedo, shading normal, depth). Kept apart from
_abi.py, which mirrors include/mi355pt.h alone."""
import ctypes as C
from ._abi import PtRenderParams, VP, fp, u32, u32p

PLANES = ("albedo", "normal", "depth")          # PtAOVBuffers' fields are <plane>_w, in this order
CHANNELS = {"albedo": 4, "normal": 4, "depth": 2}   # floats per pixel of a plane's sums


class PtAOVBuffers(C.Structure):
    _fields_ = [("albedo_w", fp), ("normal_w", fp), ("depth_w", fp)]


def buffers(planes, device=False):
    """The PtAOVBuffers of {plane: a contiguous float32 array -- with `device`: a device pointer as an integer}; a plane that is not there is NULL."""
    pointer = (lambda v: C.cast(C.c_void_p(v), fp)) if device else (lambda v: v.ctypes.data_as(fp))
    return PtAOVBuffers(*[pointer(planes[k]) if k in planes else None for k in PLANES])


# Every symbol include/mi355aov.h declares, with its signature (restype, argtypes).
ENTRY_POINTS = {
    "pt_aov_render": (C.c_int, [VP, C.POINTER(PtRenderParams), C.POINTER(PtAOVBuffers), C.c_int]),
    "pt_aov_render_samples": (C.c_int, [VP, C.POINTER(PtRenderParams), u32, u32, C.POINTER(PtAOVBuffers), C.c_int]),
    "pt_aov_pass_size": (C.c_int, [VP, C.POINTER(PtRenderParams), u32p]),
    "pt_aov_resolve": (C.c_int, [C.POINTER(PtAOVBuffers), u32, fp, fp, fp]),
}
