"""ctypes mirror of include/mi355bake.h (libmi355bake.so: ambient occlusion, bent normals, positions and normals baked into a UV atlas). Kept apart from
_abi.py, which mirrors include/mi355pt.h alone."""
import ctypes as C
from ._abi import VP, fp, u8p, u32, u32p

# Per job kind {plane: (entries per texel, dtype)}, in the order of the fields of its buffer struct (BUFFERS)
_ID, _SCALAR, _VECTOR, _SUMS = (1, "uint32"), (1, "float32"), (3, "float32"), (4, "float32")
PLANE_TABLES = {
    "bake": {"owner": _ID, "position": _VECTOR, "normal": _VECTOR, "ao_w": _SUMS},
    "transfer": {"owner": _ID, "hit_prim": _ID, "height": _SCALAR, "src_position": _VECTOR, "src_normal": _VECTOR, "tangent_normal": _VECTOR, "ao_w": _SUMS},
    "light": {"owner": _ID, "position": _VECTOR, "normal": _VECTOR, "light_w": _SUMS},
}


def _columns(kind):
    """(planes, {plane: channels}, {plane: dtype}) of a job kind"""
    table = PLANE_TABLES[kind]
    return tuple(table), {k: c for k, (c, _) in table.items()}, {k: d for k, (_, d) in table.items()}


PLANES, CHANNELS, DTYPES = _columns("bake")
TRANSFER_PLANES, TRANSFER_CHANNELS, TRANSFER_DTYPES = _columns("transfer")
LIGHT_PLANES, LIGHT_CHANNELS, LIGHT_DTYPES = _columns("light")


class PtBakeParams(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("spp", u32), ("nsamples", u32), ("cos_sample", u32), ("max_distance", C.c_float), ("sampler_type", u32),
                ("spp_per_pass", u32), ("profile", u32)]


class PtBakeBuffers(C.Structure):
    _fields_ = [("owner", u32p), ("position", fp), ("normal", fp), ("ao_w", fp)]


def buffers(planes, device=False, struct=PtBakeBuffers):
    """The PtBakeBuffers of {plane: a contiguous array of its dtype -- with `device`: a device pointer as an integer}; a plane that is not there is NULL."""
    b = struct()
    for k, (name, ctype) in enumerate(struct._fields_):
        if name in planes:
            setattr(b, name, C.cast(C.c_void_p(planes[name]), ctype) if device else planes[name].ctypes.data_as(ctype))
    return b


class PtBakeTransferParams(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("front", C.c_float), ("back", C.c_float), ("spp", u32), ("nsamples", u32), ("cos_sample", u32), ("max_distance", C.c_float),
                ("sampler_type", u32), ("spp_per_pass", u32), ("profile", u32)]


class PtBakeTransferBuffers(C.Structure):
    _fields_ = [("owner", u32p), ("hit_prim", u32p), ("height", fp), ("src_position", fp), ("src_normal", fp), ("tangent_normal", fp), ("ao_w", fp)]


def transfer_buffers(planes, device=False):
    """The PtBakeTransferBuffers of {plane: array or device pointer}, as buffers()."""
    return buffers(planes, device, PtBakeTransferBuffers)


class PtBakeLightParams(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("spp", u32), ("nsamples", u32), ("sampler_type", u32), ("spp_per_pass", u32), ("profile", u32)]


class PtBakeLightBuffers(C.Structure):
    _fields_ = [("owner", u32p), ("position", fp), ("normal", fp), ("light_w", fp)]


def light_buffers(planes, device=False):
    """The PtBakeLightBuffers of {plane: array or device pointer}, as buffers()."""
    return buffers(planes, device, PtBakeLightBuffers)


BUFFERS = {"bake": PtBakeBuffers, "transfer": PtBakeTransferBuffers, "light": PtBakeLightBuffers}

# pt_bake_sh: 28 sums per point in sh_w (27 = coefficient q, channel c at 3 q + c; the count of arrived samples), 27 coefficients per point resolved
SH_SUMS = 28
SH_COEFFICIENTS = 9


class PtBakeShParams(C.Structure):
    _fields_ = [("n_points", u32), ("row", u32), ("spp", u32), ("nsamples", u32), ("sampler_type", u32), ("spp_per_pass", u32), ("profile", u32)]


# Every symbol include/mi355bake.h declares, with its signature (restype, argtypes).
_bp, _bb = C.POINTER(PtBakeParams), C.POINTER(PtBakeBuffers)
_tp, _tb = C.POINTER(PtBakeTransferParams), C.POINTER(PtBakeTransferBuffers)
_lp, _lb = C.POINTER(PtBakeLightParams), C.POINTER(PtBakeLightBuffers)
_hp = C.POINTER(PtBakeShParams)
ENTRY_POINTS = {
    "pt_bake_render": (C.c_int, [VP, _bp, u8p, u32, _bb, C.c_int]),
    "pt_bake_render_samples": (C.c_int, [VP, _bp, u8p, u32, u32, u32, _bb, C.c_int]),
    "pt_bake_pass_size": (C.c_int, [VP, _bp, u32p]),
    "pt_bake_resolve": (C.c_int, [fp, u32, u32, fp, fp]),
    "pt_bake_dilate": (C.c_int, [VP, u32p, fp, u32, u32, u32, u32, C.c_int]),
    "pt_bake_rays": (C.c_int, [VP, _bp, u8p, u32, u32, u32p, u32p, u32p, fp, fp, fp, u8p]),
    "pt_bake_transfer": (C.c_int, [VP, VP, _tp, u8p, u32, _tb, C.c_int]),
    "pt_bake_transfer_samples": (C.c_int, [VP, VP, _tp, u8p, u32, u32, u32, _tb, C.c_int]),
    "pt_bake_transfer_pass_size": (C.c_int, [VP, VP, _tp, u32p]),
    "pt_bake_transfer_rays": (C.c_int, [VP, VP, _tp, u8p, u32, u32, u32p, u32p, u32p, fp, fp, fp, fp, fp, fp, u8p]),
    "pt_bake_light": (C.c_int, [VP, _lp, u8p, u32, u8p, u32, _lb, C.c_int]),
    "pt_bake_light_samples": (C.c_int, [VP, _lp, u8p, u32, u8p, u32, u32, u32, _lb, C.c_int]),
    "pt_bake_light_pass_size": (C.c_int, [VP, _lp, u8p, u32, u32p]),
    "pt_bake_light_resolve": (C.c_int, [fp, u32, u32, u32, fp, fp]),
    "pt_bake_light_rays": (C.c_int, [VP, _lp, u8p, u32, u8p, u32, u32, u32p, u32p, u32p, u32p, fp, fp, fp, fp, fp, fp, u8p]),
    "pt_bake_sh": (C.c_int, [VP, _hp, fp, u8p, u32, fp, C.c_int]),
    "pt_bake_sh_samples": (C.c_int, [VP, _hp, fp, u8p, u32, u32, u32, fp, C.c_int]),
    "pt_bake_sh_pass_size": (C.c_int, [VP, _hp, u8p, u32, u32p]),
    "pt_bake_sh_resolve": (C.c_int, [fp, u32, u32, u32, fp, fp]),
    "pt_bake_sh_irradiance": (C.c_int, [fp, fp, u32, fp]),
    "pt_bake_sh_rays": (C.c_int, [VP, _hp, fp, u8p, u32, u32, u32p, u32p, u32p, u32p, fp, fp, fp, fp, fp, fp, u8p]),
}
