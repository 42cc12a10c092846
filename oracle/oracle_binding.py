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


# orc_intersect's words per ray (ref_kats_shapes.cpp): name -> (first word, words, is float)
INTERSECT_FIELDS = {"hit": (0, 1, False), "prim": (1, 1, False), "inst": (2, 1, False), "t": (3, 1, True), "b": (4, 3, True), "p": (7, 3, True), "p_error": (10, 3, True),
                    "n": (13, 3, True), "wo": (16, 3, True), "uv": (19, 2, True), "dpdu": (21, 3, True), "dpdv": (24, 3, True), "sh_n": (27, 3, True),
                    "sh_dpdu": (30, 3, True), "sh_dpdv": (33, 3, True), "sh_dndu": (36, 3, True), "sh_dndv": (39, 3, True), "has_shape": (42, 1, False),
                    "shape_flip": (43, 1, False)}
INTERSECT_WORDS = 44


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
        "orc_bssrdf_eval": (i, [vp, u32, fp, fp, u32, fp, fp, u32, fp, fp, u32, fp, fp, u32, fp, u32p, fp, u32, fp, i32p, u32p, u32, fp, fp]),
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
        "orc_intersect": (i, [vp, u32, fp, fp, fp, u32p]),
    })
    return sig


class Oracle:
    def __init__(self, abi, tables_path):
        if not os.path.exists(LIB_PATH):
            build()
        self.A = abi
        self.AO = importlib.import_module("._abi_ao", abi.__package__)   # the ctypes mirror of include/mi355ao.h beside `abi`
        lib = abi.bind(C.CDLL(LIB_PATH), table=signatures(abi, self.AO))
        if lib.orc_load_tables(tables_path.encode()) != 0:
            raise RuntimeError("oracle: cannot load " + tables_path)
        self.lib = lib
        self.Scene = _scene_class(importlib.import_module(".runtime", abi.__package__).Handle)   # (the package beside `abi`: its directory's name is no identifier)

    def scene(self, scene_data):
        return self.Scene(self, scene_data)


def _assert_ok(st, what=""):
    assert st == 0, st


def _scene_class(handle):
    class OracleScene(handle):
        """orc_scene handle: runtime.Handle's entry points on the oracle, every status asserted."""
        PREFIX = LIB_PREFIX = "orc_"

        def __init__(self, orc, scene_data):
            self.O = orc
            super().__init__(orc.lib, _assert_ok, scene_data)

        @property
        def _ao(self):
            return self.O.lib

        def render(self, rp, nthreads=1, ao=None):
            """The un-normalised film (H, W, 4), as runtime.Scene.render, on `nthreads` threads."""
            return super().render(rp, ao=ao, last=nthreads)

        def seconds(self):
            return self.O.lib.orc_last_render_seconds(self.h)

        def intersect(self, o, d, tmax):
            """orc_intersect: Scene::intersect of the rays, (n, INTERSECT_WORDS) uint32 -- the hit record and the whole SurfaceInteraction (INTERSECT_FIELDS);
            a miss leaves its row zero. counters() afterwards as after trace_closest."""
            o, d, tmax = (np.ascontiguousarray(x, dtype=np.float32) for x in (o, d, tmax))
            out = np.zeros((len(tmax), INTERSECT_WORDS), np.uint32)
            self._call("intersect", self.h, len(tmax), o.ctypes.data_as(self.O.A.fp), d.ctypes.data_as(self.O.A.fp), tmax.ctypes.data_as(self.O.A.fp),
                       out.ctypes.data_as(self.O.A.u32p))
            return out

    return OracleScene
