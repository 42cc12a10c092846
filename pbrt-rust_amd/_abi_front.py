"""ctypes mirror of include/mi355front.h (libmi355front.so: the compiled .pbrt scene-file front end, host code only). Kept apart from
_abi.py, which mirrors include/mi355pt.h alone."""
import ctypes as C
from ._abi import PtRenderParams, PtSceneDesc, VP, fp, u32, u32p, u64
from ._abi_ao import PtAOParams

PTF_CHECKPOINT_MAGIC = 0x4b433550


class PtfCheckpointHeader(C.Structure):
    """The header of a range render's checkpoint file (then width * height * 4 floats of XYZW sums)."""
    _fields_ = [("magic", u32), ("version", u32), ("width", u32), ("height", u32), ("spp", u32), ("first_sample", u32), ("samples_done", u32),
                ("reserved", u32), ("params_hash", u64)]


_image = [C.c_char_p, C.c_int, C.c_int, fp]   # path, width, height, rgb

# Every symbol include/mi355front.h declares, with its signature (restype, argtypes). A ptf_scene* is a void*.
ENTRY_POINTS = {
    "ptf_parse_file": (C.c_int, [C.c_char_p, C.POINTER(VP)]),
    "ptf_parse_string": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(VP)]),
    "ptf_last_error": (C.c_char_p, []),
    "ptf_scene_desc": (C.POINTER(PtSceneDesc), [VP]),
    "ptf_render_params": (C.POINTER(PtRenderParams), [VP]),
    "ptf_output_filename": (C.c_char_p, [VP]),
    "ptf_ao_params": (C.c_int, [VP, C.POINTER(PtAOParams)]),
    "ptf_scene_destroy": (None, [VP]),
    "ptf_write_pfm": (C.c_int, _image),
    "ptf_write_image": (C.c_int, _image),
    "ptf_write_exr_channels": (C.c_int, [C.c_char_p, C.c_int, C.c_int, u32, C.POINTER(C.c_char_p), C.POINTER(fp), u32p]),
    "ptf_read_image": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_size_t]),
    "ptf_params_hash": (u64, [C.POINTER(PtRenderParams), C.POINTER(PtAOParams)]),
    "ptf_checkpoint_write": (C.c_int, [C.c_char_p, C.POINTER(PtfCheckpointHeader), fp]),
    "ptf_checkpoint_read": (C.c_int, [C.c_char_p, C.POINTER(PtfCheckpointHeader), u32p, fp]),
}

# Every symbol include/mi355front_matte.h declares (the same library; what ID mattes need of a front end).
MATTE_ENTRY_POINTS = {
    "ptf_write_exr_channels_attrs": (C.c_int, [C.c_char_p, C.c_int, C.c_int, u32, C.POINTER(C.c_char_p), C.POINTER(fp), u32p, u32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
    "ptf_prim_shape_ordinals": (C.c_int, [VP, C.POINTER(u32p), u32p]),
}
