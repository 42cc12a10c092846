"""ctypes binding of libmi355front.so, the compiled .pbrt scene-file front end (include/mi355front.h)."""
import ctypes as C
import os
import subprocess
from . import _abi as A
from . import _abi_ao as AO
from ._abi_front import ENTRY_POINTS, MATTE_ENTRY_POINTS, PTF_CHECKPOINT_MAGIC, PtfCheckpointHeader   # (re-exported: the mirror of include/mi355front.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
SAN = bool(os.environ.get("PT_SAN"))   # ASan/UBSan build of the front end (tools/san_cpu_tests.sh)
LIB_PATH = os.path.join(_HERE, "frontend", "libmi355front_san.so" if SAN else "libmi355front.so")
CLI_PATH = os.path.join(_HERE, "frontend", "mi355pbrt")


def build(verbose=False):
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "frontend")] + (["SAN=1"] if SAN else []), capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-3000:]); print(r.stderr[-3000:])
    if r.returncode != 0:
        raise RuntimeError("building libmi355front.so failed")
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = A.bind(A.bind(C.CDLL(LIB_PATH), table=ENTRY_POINTS), table=MATTE_ENTRY_POINTS)
    return _lib


class FrontScene:
    """A parsed .pbrt scene; quacks like host.SceneData (desc()) so that runtime.Scene / the oracle binding accept it."""

    def __init__(self, path=None, text=None, base_dir=None):
        L = lib()
        self.h = C.c_void_p()
        if path is not None:
            st = L.ptf_parse_file(os.fsencode(path), C.byref(self.h))
        else:
            st = L.ptf_parse_string(text.encode(), os.fsencode(base_dir) if base_dir else None, C.byref(self.h))
        if st != A.PT_OK:
            raise ValueError(L.ptf_last_error().decode(errors="replace"))

    def desc(self):
        d = lib().ptf_scene_desc(self.h).contents
        d._owner = self   # the struct points into the C++ scene: keep it alive as long as the view is
        return d

    def render_params(self):
        rp = A.PtRenderParams()
        C.memmove(C.byref(rp), lib().ptf_render_params(self.h), C.sizeof(A.PtRenderParams))
        return rp

    def ao_params(self):
        """PtAOParams of an `Integrator "ambientocclusion"` scene (render_params().integrator == PT_INTEGRATOR_AO)."""
        ao = AO.PtAOParams()
        if lib().ptf_ao_params(self.h, C.byref(ao)) != A.PT_OK: raise ValueError(lib().ptf_last_error().decode(errors="replace"))
        return ao

    def output_filename(self):
        return lib().ptf_output_filename(self.h).decode()

    @property
    def prim_group(self):
        """Per primitive, the ordinal of its Shape directive in file order (host.SceneData.prim_group's twin): a uint32 array, the `groups` of Scene.render_mattes."""
        import numpy as np
        p, n = A.u32p(), C.c_uint32()
        if lib().ptf_prim_shape_ordinals(self.h, C.byref(p), C.byref(n)) != A.PT_OK: raise ValueError(lib().ptf_last_error().decode(errors="replace"))
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint32)

    def close(self):
        if self.h:
            lib().ptf_scene_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


def read_image(path):
    """read_image (core/imageio.rs:18-40) through the compiled front end: (h, w, 3) float32, top row first."""
    import numpy as np
    L = lib(); w, h = C.c_int(), C.c_int()
    if L.ptf_read_image(os.fsencode(path), C.byref(w), C.byref(h), None, 0) != 0: raise ValueError(L.ptf_last_error().decode(errors="replace"))
    out = np.zeros((h.value, w.value, 3), np.float32)
    if L.ptf_read_image(os.fsencode(path), None, None, out.ctypes.data_as(A.fp), out.size) != 0: raise ValueError(L.ptf_last_error().decode(errors="replace"))
    return out


def write_image(path, rgb):
    """write_image (core/imageio.rs:42-60): rgb = (h, w, 3) float32, top row first; format by extension (exr, png, tga, pfm)."""
    import numpy as np
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    L = lib()
    if L.ptf_write_image(os.fsencode(path), rgb.shape[1], rgb.shape[0], rgb.ctypes.data_as(A.fp)) != 0: raise ValueError(L.ptf_last_error().decode(errors="replace"))


def write_exr_channels(path, channels, attributes=()):
    """An EXR file of FLOAT channels: `channels` = {name: (h, w) float32 array}, written in the byte-wise sorted order of the names; `attributes` = (name, value)
    pairs of strings, written as string attributes after the required ones."""
    import numpy as np
    names = sorted(channels, key=lambda s: s.encode())
    arrs = [np.ascontiguousarray(channels[k], dtype=np.float32) for k in names]
    h, w = arrs[0].shape
    if any(a.shape != (h, w) for a in arrs): raise ValueError("write_exr_channels: the channels differ in shape")
    n, m = len(names), len(attributes)
    cn = (C.c_char_p * n)(*[s.encode() for s in names])
    ptrs = (A.fp * n)(*[a.ctypes.data_as(A.fp) for a in arrs])
    strides = (C.c_uint32 * n)(*([1] * n))
    an = (C.c_char_p * max(m, 1))(*[k.encode() for k, _ in attributes]); av = (C.c_char_p * max(m, 1))(*[v.encode() for _, v in attributes])
    L = lib()
    if L.ptf_write_exr_channels_attrs(os.fsencode(path), w, h, n, cn, ptrs, strides, m, an, av) != A.PT_OK: raise ValueError(L.ptf_last_error().decode(errors="replace"))


def checkpoint_header(rp, ao=None, first_sample=0, samples_done=0):
    """The header of the job (rp, ao) rendered from `first_sample` on."""
    cb = rp.cropped_pixel_bounds
    return PtfCheckpointHeader(PTF_CHECKPOINT_MAGIC, 1, cb[2] - cb[0], cb[3] - cb[1], rp.spp, first_sample, samples_done, 0,
                               lib().ptf_params_hash(C.byref(rp), C.byref(ao) if ao is not None else None))


def write_checkpoint(path, header, film):
    import numpy as np
    film = np.ascontiguousarray(film, dtype=np.float32)
    assert film.size == header.width * header.height * 4
    if lib().ptf_checkpoint_write(os.fsencode(path), C.byref(header), film.ctypes.data_as(A.fp)) != A.PT_OK: raise ValueError(lib().ptf_last_error().decode(errors="replace"))


def read_checkpoint(path, expect):
    """(samples done, film (h, w, 4)) of the checkpoint at `path` for the job `expect` describes; (0, zeros) when there is none; ValueError when it is of another job."""
    import numpy as np
    film = np.zeros((expect.height, expect.width, 4), np.float32); done = C.c_uint32()
    if lib().ptf_checkpoint_read(os.fsencode(path), C.byref(expect), C.byref(done), film.ctypes.data_as(A.fp)) != A.PT_OK: raise ValueError(lib().ptf_last_error().decode(errors="replace"))
    return done.value, film
