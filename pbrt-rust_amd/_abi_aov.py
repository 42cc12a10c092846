"""ctypes mirror of include/mi355aov.h (libmi355aov.so: the feature buffers for denoising -- albedo, shading normal, depth). Kept apart from
_abi.py, which mirrors include/mi355pt.h alone."""
import ctypes as C
import numpy as np
from ._abi import PtRenderParams, VP, fp, u32, u32p

PLANES = ("albedo", "normal", "depth")          # PtAOVBuffers' fields are <plane>_w, in this order
CHANNELS = {"albedo": 4, "normal": 4, "depth": 2}   # floats per pixel of a plane's sums


class PtAOVBuffers(C.Structure):
    _fields_ = [("albedo_w", fp), ("normal_w", fp), ("depth_w", fp)]


def buffers(planes, device=False):
    """The PtAOVBuffers of {plane: a contiguous float32 array -- with `device`: a device pointer as an integer}; a plane that is not there is NULL."""
    pointer = (lambda v: C.cast(C.c_void_p(v), fp)) if device else (lambda v: v.ctypes.data_as(fp))
    return PtAOVBuffers(*[pointer(planes[k]) if k in planes else None for k in PLANES])


# ---- ID mattes ----
PT_MATTE_SLOTS = 8
MATTE_LAYERS = ("material", "instance", "group")   # PtMatteLayer: PtMatteBuffers.layer's indices
CRYPTO_LAYER_NAMES = {"material": "CryptoMaterial", "instance": "CryptoInstance", "group": "CryptoGroup"}


class PtMattePixel(C.Structure):
    _fields_ = [("id", u32 * PT_MATTE_SLOTS), ("w", C.c_float * PT_MATTE_SLOTS), ("n_ids", u32), ("w_total", C.c_float), ("w_other", C.c_float), ("reserved", u32)]


class PtMatteBuffers(C.Structure):
    _fields_ = [("layer", C.POINTER(PtMattePixel) * 3), ("prim_group", u32p), ("n_prims", u32)]


# PtMattePixel as a numpy structured dtype: a table of a film is an (H, W) array of it, all zero = empty
MATTE_DTYPE = np.dtype([("id", "<u4", (PT_MATTE_SLOTS,)), ("w", "<f4", (PT_MATTE_SLOTS,)), ("n_ids", "<u4"), ("w_total", "<f4"), ("w_other", "<f4"), ("reserved", "<u4")])
mp = C.POINTER(PtMattePixel)


def matte_buffers(tables, groups=None, device=False):
    """The PtMatteBuffers of {layer: a contiguous MATTE_DTYPE array -- with `device`: a device pointer as an integer}; a layer that is not there is NULL. `groups`: a
    contiguous uint32 array, the caller's id of every primitive (host memory in either case). The arrays must outlive the call the result is handed to."""
    pointer = (lambda v: C.cast(C.c_void_p(v), mp)) if device else (lambda v: v.ctypes.data_as(mp))
    b = PtMatteBuffers()
    for k, name in enumerate(MATTE_LAYERS):
        if name in tables:
            b.layer[k] = pointer(tables[name])
    if groups is not None:
        b.prim_group = groups.ctypes.data_as(u32p); b.n_prims = len(groups)
    return b


# Every symbol include/mi355aov.h declares, with its signature (restype, argtypes).
ENTRY_POINTS = {
    "pt_aov_render": (C.c_int, [VP, C.POINTER(PtRenderParams), C.POINTER(PtAOVBuffers), C.c_int]),
    "pt_aov_render_samples": (C.c_int, [VP, C.POINTER(PtRenderParams), u32, u32, C.POINTER(PtAOVBuffers), C.c_int]),
    "pt_aov_pass_size": (C.c_int, [VP, C.POINTER(PtRenderParams), u32p]),
    "pt_aov_resolve": (C.c_int, [C.POINTER(PtAOVBuffers), u32, fp, fp, fp]),
    "pt_matte_render": (C.c_int, [VP, C.POINTER(PtRenderParams), C.POINTER(PtMatteBuffers), C.c_int]),
    "pt_matte_render_samples": (C.c_int, [VP, C.POINTER(PtRenderParams), u32, u32, C.POINTER(PtMatteBuffers), C.c_int]),
    "pt_matte_pass_size": (C.c_int, [VP, C.POINTER(PtRenderParams), u32p]),
    "pt_matte_resolve": (C.c_int, [mp, u32, u32, u32p, fp]),
    "pt_matte_mask": (C.c_int, [VP, mp, C.c_int, u32, u32p, u32, fp, C.c_int]),
}
