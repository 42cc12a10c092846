"""ctypes mirror of include/mi355ao.h (libmi355ao.so: the ambient-occlusion integrator). Kept apart from _abi.py, which mirrors
include/mi355pt.h alone."""
import ctypes as C
from ._abi import PtRenderParams, VP, u32, u32p

PT_INTEGRATOR_AO = 2   # PtRenderParams.integrator of an "ambientocclusion" scene: rendered by pt_ao_render, not by pt_render


class PtAOParams(C.Structure):
    _fields_ = [("nsamples", u32), ("cos_sample", u32)]


# Every symbol include/mi355ao.h declares, with its signature (restype, argtypes).
ENTRY_POINTS = {
    "pt_ao_render": (C.c_int, [VP, C.POINTER(PtRenderParams), C.POINTER(PtAOParams), VP, C.c_int]),
    "pt_ao_render_samples": (C.c_int, [VP, C.POINTER(PtRenderParams), C.POINTER(PtAOParams), u32, u32, VP, C.c_int]),
    "pt_ao_pass_size": (C.c_int, [VP, C.POINTER(PtRenderParams), C.POINTER(PtAOParams), u32p]),
}
