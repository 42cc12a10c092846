"""ctypes binding of the CPU oracle (TEST INFRASTRUCTURE: imported only by tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg)."""
import ctypes as C
import importlib
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SAN = bool(os.environ.get("PT_SAN"))   # ASan/UBSan build of the oracle (tools/san_cpu_tests.sh preloads the sanitizer runtimes)
LIB_PATH = os.path.join(_HERE, "liboracle_san.so" if SAN else "liboracle.so")


def build(verbose=False):
    r = subprocess.run(["make", "-C", _HERE] + (["SAN=1"] if SAN else []), capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-3000:]); print(r.stderr[-3000:])
    if r.returncode != 0:
        raise RuntimeError("building liboracle.so failed")
    return LIB_PATH


# orc_* functions that mirror a pt_* entry point of include/mi355pt.h: their signature is the one _abi.ENTRY_POINTS declares
_MIRRORED = ("pt_scene_create", "pt_scene_destroy", "pt_scene_bvh_info", "pt_scene_bvh_read", "pt_get_counters", "pt_film_resolve",
             "pt_trace_closest", "pt_trace_any", "pt_sobol_samples", "pt_halton_samples", "pt_camera_rays")


def signatures(A, AO):
    """{name: (restype, argtypes)} of every orc_* function liboracle.so exports (tests/test_oracle_binding.py holds the two sets equal).
    A / AO: the ctypes mirrors of include/mi355pt.h / mi355ao.h."""
    f, d, i, u32, u64, vp = C.c_float, C.c_double, C.c_int, C.c_uint32, C.c_uint64, C.c_void_p
    fp, u32p, i32p = A.fp, A.u32p, A.i32p
    ip, dp, rpp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(A.PtRenderParams)
    tp, sp = C.POINTER(A.PtBSSRDFTable), C.POINTER(A.PtSphere)
    sig = {k.replace("pt_", "orc_", 1): A.ENTRY_POINTS[k] for k in _MIRRORED}
    sig.update({
        # the render path and its parity API (ref_render.cpp)
        "orc_load_tables": (i, [C.c_char_p]),
        "orc_render": (i, [vp, rpp, fp, i]),
        "orc_ao_render": (i, [vp, rpp, C.POINTER(AO.PtAOParams), fp, i]),
        "orc_last_render_seconds": (d, [vp]),
        "orc_tmax_raises": (u64, []),      # triangle hits that raised t_max (ref_scene.h g_tmax_raises)
        "orc_reset_tmax_raises": (None, []),
        # reference-test loops (ref_kats.cpp)
        "orc_test_efloat": (i, [i, i, ip]),
        "orc_test_float_bits": (i, [i, ip]),
        "orc_test_scrambled_radical_inverse": (i, [i, dp]),
        "orc_test_bitops": (i, []),
        "orc_test_generator_matrix": (i, []),
        "orc_test_hg_sampling_match": (d, []),
        "orc_test_hg_orientation": (None, [f, ip, ip]),
        "orc_test_hg_normalized": (None, [dp]),
        # function probes (ref_kats.cpp)
        "orc_sobol_sample_float": (f, [u64, i, u32]),
        "orc_radical_inverse": (f, [i, u64]),
        "orc_radical_inverse_any": (f, [u32, u64]),
        "orc_halton_permutation": (u32, [u32, C.POINTER(C.c_uint16)]),
        "orc_next_float_up": (f, [f]),
        "orc_next_float_down": (f, [f]),
        "orc_find_interval": (i, [i, fp, f]),
        "orc_rng_u32_stream": (u32, [u64, i, u32, u32p, fp]),
        "orc_dist1d_sample_discrete": (i, [fp, i, f, fp, fp]),
        "orc_dist1d_discrete_pdf": (f, [fp, i, i]),
        "orc_dist1d_sample_continuous": (f, [fp, i, f, fp, ip]),
        "orc_dm_sin": (f, [f]),
        "orc_dm_cos": (f, [f]),
        "orc_dm_acos": (f, [f]),
        "orc_dm_atan2": (f, [f, f]),
        "orc_dm_log": (f, [f]),
        "orc_offset_ray_origin": (None, [fp] * 5),
        "orc_bssrdf_sr": (i, [tp, fp, fp, f, u32, fp, fp, fp]),
        "orc_bssrdf_sample_sr": (i, [tp, fp, fp, f, i, u32, fp, fp]),
        "orc_catmull_rom_weights": (i, [i, fp, f, ip, fp]),
        "orc_bssrdf_sw": (f, [f, f]),
        "orc_light_sample_li": (i, [vp, u32, fp, fp, fp, u32, fp, fp, fp, fp]),
        "orc_light_pdf_li": (i, [vp, u32, fp, fp, fp, u32, fp, fp]),
        "orc_bsdf_eval": (i, [vp, u32, u32, fp, fp, fp, fp, fp, fp, fp, fp, i32p, i32p]),
        # shape loops and probes (ref_kats_shapes.cpp)
        "orc_test_triangle_sampling": (i, [i, i, dp]),
        "orc_test_triangle_solid_angle": (i, [i, i, dp]),
        "orc_test_sphere_solid_angle": (i, [sp, i, dp]),
        "orc_test_disk_solid_angle": (i, [sp, i, dp]),
        "orc_test_triangle_watertight": (i, [i, i, fp, u32p, fp, fp, ip]),
        "orc_test_partial_sphere_normal": (i, [i, ip, dp]),
        "orc_test_triangle_reintersect": (i, [i, i, ip]),
        "orc_test_sphere_reintersect": (i, [i, i, i, ip]),
        "orc_tri_intersect": (i, [vp, u32, fp, fp, f, fp, fp, fp, fp, fp]),
        "orc_tri_intersect_p": (i, [vp, u32, fp, fp, f]),
    })
    return sig


class Oracle:
    def __init__(self, abi, tables_path):
        if not os.path.exists(LIB_PATH):
            build()
        self.A = abi
        self.AO = importlib.import_module("._abi_ao", abi.__package__)   # the ctypes mirror of include/mi355ao.h beside `abi`
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in signatures(abi, self.AO).items():
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
        if lib.orc_load_tables(tables_path.encode()) != 0:
            raise RuntimeError("oracle: cannot load " + tables_path)
        self.lib = lib

    def scene(self, scene_data):
        return OracleScene(self, scene_data)


def _fp(A, a):
    return a.ctypes.data_as(A.fp)


class OracleScene:
    def __init__(self, orc, scene_data):
        self.O = orc; self.A = orc.A; self.data = scene_data
        self.h = C.c_void_p()
        d = scene_data.desc()
        st = orc.lib.orc_scene_create(C.byref(d), C.byref(self.h))
        assert st == 0, st

    def close(self):
        if self.h:
            self.O.lib.orc_scene_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass

    def bvh(self):
        A = self.A
        nn, npr = C.c_uint32(), C.c_uint32()
        self.O.lib.orc_scene_bvh_info(self.h, C.byref(nn), C.byref(npr))
        nodes = (A.PtBVHNode * nn.value)(); ordered = np.zeros(npr.value, dtype=np.uint32)
        self.O.lib.orc_scene_bvh_read(self.h, nodes, ordered.ctypes.data_as(A.u32p))
        return nodes, ordered

    def render(self, rp, nthreads=1, ao=None):
        """The un-normalised film (H, W, 4), as runtime.Scene.render: rp.integrator == PT_INTEGRATOR_AO renders with orc_ao_render
        and `ao` (a PtAOParams), else the scene's own (scene_data.ao_params())."""
        cb = rp.cropped_pixel_bounds
        w, h = cb[2] - cb[0], cb[3] - cb[1]
        film = np.zeros((h, w, 4), dtype=np.float32)
        if rp.integrator == self.O.AO.PT_INTEGRATOR_AO:
            ao = self.data.ao_params() if ao is None else ao
            st = self.O.lib.orc_ao_render(self.h, C.byref(rp), C.byref(ao), _fp(self.A, film), nthreads)
        else:
            st = self.O.lib.orc_render(self.h, C.byref(rp), _fp(self.A, film), nthreads)
        assert st == 0, st
        return film

    def seconds(self):
        return self.O.lib.orc_last_render_seconds(self.h)

    def resolve(self, film, scale=1.0):
        out = np.zeros(film.shape[:-1] + (3,), dtype=np.float32)
        self.O.lib.orc_film_resolve(_fp(self.A, film), film.size // 4, scale, _fp(self.A, out))
        return out

    def counters(self):
        c = self.A.PtCounters()
        self.O.lib.orc_get_counters(self.h, C.byref(c))
        return c.as_dict()

    def trace_closest(self, o, d, tmax):
        A = self.A
        o, d, tmax = (np.ascontiguousarray(x, dtype=np.float32) for x in (o, d, tmax))
        n = len(tmax)
        prim = np.zeros(n, np.uint32); t = np.zeros(n, np.float32); b = np.zeros((n, 3), np.float32)
        self.O.lib.orc_trace_closest(self.h, n, _fp(A, o), _fp(A, d), _fp(A, tmax), prim.ctypes.data_as(A.u32p), _fp(A, t), _fp(A, b))
        return prim, t, b

    def trace_any(self, o, d, tmax):
        A = self.A
        o, d, tmax = (np.ascontiguousarray(x, dtype=np.float32) for x in (o, d, tmax))
        n = len(tmax)
        hit = np.zeros(n, np.uint8)
        self.O.lib.orc_trace_any(self.h, n, _fp(A, o), _fp(A, d), _fp(A, tmax), hit.ctypes.data_as(A.u8p))
        return hit
