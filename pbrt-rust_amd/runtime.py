"""ctypes binding of libmi355pt.so (the HIP product library).  Fails loudly when the
extension is missing: there is NO CPU fallback behind this module."""
import ctypes as C
import math
import os
import subprocess
import numpy as np
from . import _abi as A
from . import _abi_ao as AO
from . import _abi_aov as AOV
from . import _abi_dn as DN
from . import _abi_bake as BAKE

_HERE = os.path.dirname(os.path.abspath(__file__))
# The HIP libraries, in build order: the product library, then those linked against it. name: (directory, file, ctypes mirror, header under include/).
# What builds them, finds them, loads them (Library) and checks their exports (__graft_entry__.build) reads this table.
LIBRARIES = {
    "pt": ("csrc", "libmi355pt.so", A, "mi355pt.h"),
    "ao": ("ao", "libmi355ao.so", AO, "mi355ao.h"),          # the ambient-occlusion integrator
    "aov": ("aov", "libmi355aov.so", AOV, "mi355aov.h"),     # the feature buffers for denoising
    "dn": ("denoise", "libmi355dn.so", DN, "mi355dn.h"),     # the a-trous denoiser over half films and feature buffers
    "bake": ("bake", "libmi355bake.so", BAKE, "mi355bake.h"),   # AO, bent normals, positions and normals baked into a UV atlas
}
LIB_PATHS = {name: os.path.join(_HERE, sub, file) for name, (sub, file, _, _) in LIBRARIES.items()}
LIB_PATHS["pt"] = os.environ.get("PT_LIB_PATH") or LIB_PATHS["pt"]   # PT_LIB_PATH: kernel-variant experiments
LIB_PATH, AO_LIB_PATH, AOV_LIB_PATH, DN_LIB_PATH = (LIB_PATHS[name] for name in ("pt", "ao", "aov", "dn"))
TABLES_PATH = os.path.join(_HERE, "data", "sobol_tables.bin")


def build_library(verbose=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU): the libraries of LIBRARIES, in its order."""
    for sub, file, _, _ in LIBRARIES.values():
        r = subprocess.run(["make", "-C", os.path.join(_HERE, sub), "-j8"], capture_output=True, text=True)
        if verbose or r.returncode != 0:
            print(r.stdout[-4000:]); print(r.stderr[-4000:])
        if r.returncode != 0:
            raise RuntimeError(f"building {file} failed")
    return LIB_PATH


class PtError(RuntimeError):
    pass


class Library:
    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise PtError(f"{path} not found: build it with __graft_entry__.build() (no CPU fallback exists)")
        self.lib = A.bind(C.CDLL(path), strict=not os.environ.get("PT_LIB_PATH"))   # (PT_LIB_PATH: a kernel-variant library of an A/B run, possibly built from an older tree)

    def __getattr__(self, name):
        """.ao, .aov, .dn, .bake: a library of LIBRARIES linked against the product library, loaded and bound on first use (and then an attribute like any other)."""
        if name == "pt" or name not in LIBRARIES:
            raise AttributeError(name)
        path = LIB_PATHS[name]
        if not os.path.exists(path):
            raise PtError(f"{path} not found: build it with __graft_entry__.build() (no CPU fallback exists)")
        setattr(self, name, A.bind(C.CDLL(path), table=LIBRARIES[name][2].ENTRY_POINTS))
        return getattr(self, name)

    def check(self, st, what=""):
        if st != A.PT_OK:
            raise PtError(f"{what} failed: status {st}: {self.lib.pt_last_error().decode(errors='replace')}")

    def init(self, device=0):
        self.check(self.lib.pt_init(device), "pt_init")

    def set_trace_exact(self, exact):
        """True: the two-wide BVH walk whose `bvh_nodes_visited` is the reference's counter; False (default): the four-wide production walk
        (same hits, films and other counters). Returns the previous setting."""
        return bool(self.lib.pt_set_trace_exact(1 if exact else 0))


_lib = None


def load_library():
    global _lib
    if _lib is None:
        _lib = Library()
    return _lib


def _fptr(a):
    return a.ctypes.data_as(A.fp)


def _sampler_code(sampler):
    return {"sobol": A.PT_SAMPLER_SOBOL, "halton": A.PT_SAMPLER_HALTON}[sampler]


# what pt_bake_light_rays and pt_bake_sh_rays return per light sample, in their order: (key, is a 3-vector)
_LIGHT_SAMPLE = (("wi", True), ("pdf", False), ("Li", True), ("E", True), ("o", True), ("d", True))


def film_shape(rp):
    """(h, w) of the film of the job `rp`: its cropped pixel window."""
    cb = rp.cropped_pixel_bounds
    return cb[3] - cb[1], cb[2] - cb[0]


def _device_zeros(*shapes):
    """Zeroed float32 torch tensors of `shapes` on the device, there to be added to."""
    import torch
    out = [torch.zeros(s, dtype=torch.float32, device="cuda") for s in shapes]
    torch.cuda.synchronize()   # (the library renders on its own stream: the zeroed buffers must be there before it adds to them)
    return out


def default_denoise_params(lib=None):
    """pt_denoise_default_params: a PtDenoiseParams to adjust and hand to Scene.denoise / Scene.render_denoised."""
    p = DN.PtDenoiseParams()
    (lib or load_library()).dn.pt_denoise_default_params(C.byref(p))
    return p


def resolve_aov(sums, lib=None):
    """pt_aov_resolve of the sums Scene.render_aov returns: {"albedo": (H, W, 3) = sum / weight of all samples, "normal": (H, W, 3) = the normalised sum,
    "depth": (H, W) = sum / weight of the hits}, 0 where the weight is 0; the planes `sums` holds."""
    lib = lib or load_library()
    sums = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sums.items()}
    shape = next(iter(sums.values())).shape[:2]
    out = {k: np.zeros(shape + ((3,) if k != "depth" else ()), dtype=np.float32) for k in sums}
    lib.check(lib.aov.pt_aov_resolve(C.byref(AOV.buffers(sums)), shape[0] * shape[1], *[_fptr(out[k]) if k in out else None for k in AOV.PLANES]), "pt_aov_resolve")
    return out


def resolve_mattes(tables, ranks=6, lib=None):
    """pt_matte_resolve of the tables Scene.render_mattes returns: {layer: (ids (H, W, ranks) uint32, coverage (H, W, ranks) float32)} -- per pixel the `ranks` (1 .. 8)
    heaviest slots, by weight descending and ties to the lower id, coverage = w / w_total; id 0 and coverage 0 where a rank has no slot or the pixel no weight."""
    lib = lib or load_library()
    out = {}
    for layer, table in tables.items():
        table = np.ascontiguousarray(table, dtype=AOV.MATTE_DTYPE)
        ids = np.zeros(table.shape + (max(ranks, 0),), np.uint32); cov = np.zeros(ids.shape, np.float32)
        lib.check(lib.aov.pt_matte_resolve(table.ctypes.data_as(AOV.mp), table.size, ranks, ids.ctypes.data_as(A.u32p), _fptr(cov)), "pt_matte_resolve")
        out[layer] = (ids, cov)
    return out


def resolve_bake(ao_w, spp, lib=None):
    """pt_bake_resolve of the ao_w sums Scene.bake returns, (H, W, 4): (ao (H, W) = sum w / (spp * pi): 1 for an open surface under cosine sampling, bent (H, W, 3) = the normalised sum of the unoccluded
    directions), 0 where nothing was added."""
    lib = lib or load_library()
    ao_w = np.ascontiguousarray(ao_w, dtype=np.float32)
    shape = ao_w.shape[:-1]
    ao = np.zeros(shape, np.float32); bent = np.zeros(shape + (3,), np.float32)
    lib.check(lib.bake.pt_bake_resolve(_fptr(ao_w), ao_w.size // 4, spp, _fptr(ao), _fptr(bent)), "pt_bake_resolve")
    return ao, bent


def resolve_lightmap(light_w, spp, nsamples, lib=None):
    """pt_bake_light_resolve of the light_w sums Scene.bake_light returns, (H, W, 4): (irradiance (H, W, 3) = sum E / spp, reached (H, W) = the fraction of the
    spp * nsamples light samples of a texel that arrived), 0 where nothing was added."""
    lib = lib or load_library()
    light_w = np.ascontiguousarray(light_w, dtype=np.float32)
    shape = light_w.shape[:-1]
    irradiance = np.zeros(shape + (3,), np.float32); reached = np.zeros(shape, np.float32)
    lib.check(lib.bake.pt_bake_light_resolve(_fptr(light_w), light_w.size // 4, spp, nsamples, _fptr(irradiance), _fptr(reached)), "pt_bake_light_resolve")
    return irradiance, reached


def resolve_sh(sh_w, spp, nsamples, lib=None):
    """pt_bake_sh_resolve of the sh_w sums Scene.bake_sh returns, (n, 28): (sh (n, 9, 3) = the order-2 SH coefficients of the direct incident radiance per
    colour channel, reached (n,) = the fraction of the spp * nsamples light samples of a point that arrived), 0 where nothing was added."""
    lib = lib or load_library()
    sh_w = np.ascontiguousarray(sh_w, dtype=np.float32)
    n = sh_w.size // BAKE.SH_SUMS
    sh = np.zeros((n, BAKE.SH_COEFFICIENTS, 3), np.float32); reached = np.zeros(n, np.float32)
    lib.check(lib.bake.pt_bake_sh_resolve(_fptr(sh_w), n, spp, nsamples, _fptr(sh), _fptr(reached)), "pt_bake_sh_resolve")
    return sh, reached


def sh_irradiance(sh, normals, lib=None):
    """pt_bake_sh_irradiance: the irradiance (n, 3) a surface of unit normal normals[i] receives under the coefficients sh[i] ((n, 9, 3), as resolve_sh returns
    them; one entry is used for every normal). Not clamped: an order-2 fit can go slightly negative."""
    lib = lib or load_library()
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    sh = np.asarray(sh, dtype=np.float32).reshape(-1, BAKE.SH_COEFFICIENTS, 3)
    if len(sh) == 1 and len(normals) != 1:
        sh = np.broadcast_to(sh, (len(normals), BAKE.SH_COEFFICIENTS, 3))
    if len(sh) != len(normals):
        raise ValueError(f"sh_irradiance: {len(sh)} sets of coefficients, {len(normals)} normals")
    sh = np.ascontiguousarray(sh)
    out = np.zeros((len(normals), 3), np.float32)
    lib.check(lib.bake.pt_bake_sh_irradiance(_fptr(sh), _fptr(normals), len(normals), _fptr(out)), "pt_bake_sh_irradiance")
    return out


def encode_normal_map(tangent_normal, covered):
    """The tangent_normal plane of Scene.bake_transfer, (H, W, 3), as a normal-map image: n * 0.5 + 0.5 where `covered` ((H, W) bool: the texels with a detail hit, or
    those a dilation filled), the flat normal (0.5, 0.5, 1) elsewhere. float32."""
    n = np.asarray(tangent_normal, dtype=np.float32)
    flat = np.array([0.5, 0.5, 1.0], np.float32)
    return np.where(np.asarray(covered, bool)[..., None], n * np.float32(0.5) + np.float32(0.5), flat).astype(np.float32)


def murmur3_32(data, seed=0):
    """MurmurHash3_x86_32 of a bytes object."""
    c1, c2, M = 0xcc9e2d51, 0x1b873593, 0xffffffff
    rotl = lambda v, r: ((v << r) | (v >> (32 - r))) & M
    h, n = seed & M, len(data)
    for i in range(0, n - n % 4, 4):
        k = int.from_bytes(data[i:i + 4], "little")
        k = (rotl((k * c1) & M, 15) * c2) & M
        h = (rotl(h ^ k, 13) * 5 + 0xe6546b64) & M
    tail = data[n - n % 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        h ^= (rotl((k * c1) & M, 15) * c2) & M
    h ^= n
    h ^= h >> 16; h = (h * 0x85ebca6b) & M
    h ^= h >> 13; h = (h * 0xc2b2ae35) & M
    return h ^ (h >> 16)


def cryptomatte_id(name):
    """The Cryptomatte id of a name: MurmurHash3_32 of its UTF-8 bytes (seed 0), and -- the id travels as a float32 bit pattern -- with bit 23 flipped where the
    exponent bits are all 0 or all 1, so that it is neither a denormal nor an infinity or NaN."""
    h = murmur3_32(name.encode("utf-8"))
    return h ^ (1 << 23) if (h >> 23) & 255 in (0, 255) else h


def default_matte_name(layer, raw_id):
    """The name write_cryptomatte gives the raw id of a layer when the caller has none: material<i>; world for top-level geometry and instance<i> for the instance
    layer's id i = 1 + the instance's index; group<i>."""
    if layer == "instance":
        return "world" if raw_id == 0 else "instance%d" % raw_id
    return "%s%d" % (layer, raw_id)


def write_cryptomatte(path, tables, names=None, ranks=6, lib=None):
    """The tables of Scene.render_mattes as a Cryptomatte EXR. Per layer L (CryptoMaterial, CryptoInstance, CryptoGroup) the FLOAT channels L00.R/G/B/A, L01. ...: two
    ranks per RGBA set, R and B the id's float32 bit pattern, G and A its coverage (pt_matte_resolve's ranks); and the string attributes cryptomatte/<key>/name, /hash
    ("MurmurHash3_32"), /conversion ("uint32_to_float32") and /manifest (JSON {name: "%08x" of its id}), <key> the first 7 hex digits of the layer name's id.
    `names` = {layer: {raw id: name}}; ids without a name get default_matte_name. The written id of a raw id is cryptomatte_id of its name."""
    import json
    from . import frontend
    names = names or {}
    channels, attributes = {}, []
    for layer, (ids, cov) in resolve_mattes(tables, ranks, lib).items():
        L = AOV.CRYPTO_LAYER_NAMES[layer]
        table = np.asarray(tables[layer])
        slot_used = np.arange(AOV.PT_MATTE_SLOTS)[None, None, :] < table["n_ids"][..., None]
        raw = sorted(set(int(v) for v in np.unique(table["id"][slot_used])) | set(names.get(layer, {})))
        name_of = {i: names.get(layer, {}).get(i, default_matte_name(layer, i)) for i in raw}
        hashed = {i: cryptomatte_id(n) for i, n in name_of.items()}
        lut_keys = np.array(raw, np.uint32); lut_vals = np.array([hashed[i] for i in raw], np.uint32)
        ranked = cov != 0.0   # (a rank without a slot is id 0, coverage 0: it stays 0.0 in the file)
        written = np.zeros(ids.shape, np.uint32)
        if len(raw):
            written[ranked] = lut_vals[np.searchsorted(lut_keys, ids[ranked])]
        bits = written.view(np.float32)
        for r in range(ranks + ranks % 2):
            base = "%s%02d." % (L, r // 2)
            zero = np.zeros(ids.shape[:2], np.float32)
            channels[base + "RB"[r % 2]] = bits[..., r] if r < ranks else zero
            channels[base + "GA"[r % 2]] = cov[..., r] if r < ranks else zero
        key = "cryptomatte/%s/" % ("%08x" % cryptomatte_id(L))[:7]
        attributes += [(key + "name", L), (key + "hash", "MurmurHash3_32"), (key + "conversion", "uint32_to_float32"),
                       (key + "manifest", json.dumps({name_of[i]: "%08x" % hashed[i] for i in raw}, sort_keys=True))]
    frontend.write_exr_channels(path, channels, attributes)


class Handle:
    """A scene handle of a library whose C functions carry a prefix: `pt_` (Scene), `pt_multi_` (MultiScene), `orc_` (the CPU oracle's scene).
    `cdll` holds the functions, `check(status, what)` raises on a status other than PT_OK, `extra` goes between the description and the handle in
    <PREFIX>scene_create. The AO integrator's functions live in `self._ao` (None: the handle has no AO integrator)."""
    PREFIX = "pt_"
    LIB_PREFIX = "pt_"   # of the functions that take no handle (film_resolve)
    _ao = None

    def __init__(self, cdll, check, scene_data, *extra):
        self._lib, self._check = cdll, check
        self.data = scene_data
        self.h = C.c_void_p()
        d = scene_data.desc()
        self._call("scene_create", C.byref(d), *extra, C.byref(self.h))

    def _call(self, name, *args, lib=None):
        name = self.PREFIX + name
        self._check(getattr(lib or self._lib, name)(*args), name)

    def close(self):
        if self.h:
            getattr(self._lib, self.PREFIX + "scene_destroy")(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass

    def bvh(self):
        nn, npr = C.c_uint32(), C.c_uint32()
        self._call("scene_bvh_info", self.h, C.byref(nn), C.byref(npr))
        nodes = (A.PtBVHNode * nn.value)(); ordered = np.zeros(npr.value, dtype=np.uint32)
        self._call("scene_bvh_read", self.h, nodes, ordered.ctypes.data_as(A.u32p))
        return nodes, ordered

    def render(self, rp, film=None, device_ptr=None, ao=None, last=None, samples=None):
        """Returns the un-normalised film (H, W, 4) = XYZ sums + weight sum, or None when it went to `device_ptr`. rp.integrator ==
        PT_INTEGRATOR_AO renders with <PREFIX>ao_render: `ao` (a PtAOParams), else the scene's own (scene_data.ao_params()).
        `last`: the call's final argument, by default the product library's `film_on_device`.
        `samples` = (first, n): sample numbers [first, first + n) of the job of rp.spp samples per pixel (<PREFIX>render_samples), ADDED to `film`; unset: the whole job."""
        args, lib, name = [self.h, C.byref(rp)], self._lib, "render"
        if rp.integrator == AO.PT_INTEGRATOR_AO and self._ao is not None:
            ao = self.data.ao_params() if ao is None else ao
            args.append(C.byref(ao)); lib, name = self._ao, "ao_render"
        if samples is not None:
            first, n = samples
            args += [first, n]; name += "_samples"
        return self._film_call(name, args, rp, film, device_ptr, last, lib)

    def _film_call(self, name, args, rp, film, device_ptr, last, lib):
        """The tail of a render call that ADDS to a film: to the device film at `device_ptr` (returns None), else to the host array `film`, made when None and returned."""
        if device_ptr is not None:
            self._call(name, *args, C.c_void_p(device_ptr), 1, lib=lib); return None
        if film is None:
            film = np.zeros(film_shape(rp) + (4,), dtype=np.float32)
        film_type = getattr(lib, self.PREFIX + name).argtypes[-2]   # void* in the product library, float* in the oracle
        self._call(name, *args, film.ctypes.data_as(film_type), 0 if last is None else last, lib=lib)
        return film

    def resolve(self, film, scale=1.0):
        film = np.ascontiguousarray(film, dtype=np.float32)
        out = np.zeros(film.shape[:-1] + (3,), dtype=np.float32)
        name = self.LIB_PREFIX + "film_resolve"
        self._check(getattr(self._lib, name)(_fptr(film), film.size // 4, scale, _fptr(out)), name)
        return out

    def counters(self):
        c = A.PtCounters()
        self._call("get_counters", self.h, C.byref(c))
        return c.as_dict()

    def kernel_stats(self, *replica):
        arr = (A.PtKernelStat * 32)(); n = C.c_uint32()
        self._call("get_kernel_stats", self.h, *replica, arr, 32, C.byref(n))
        text = lambda v: v.decode() if isinstance(v, bytes) else v
        return [{k: text(getattr(arr[i], k)) for k, _ in A.PtKernelStat._fields_} for i in range(n.value)]

    def trace_closest(self, o, d, tmax):
        o, d, tmax = (np.ascontiguousarray(x, dtype=np.float32) for x in (o, d, tmax))
        n = len(tmax)
        prim = np.zeros(n, np.uint32); t = np.zeros(n, np.float32); b = np.zeros((n, 3), np.float32)
        self._call("trace_closest", self.h, n, _fptr(o), _fptr(d), _fptr(tmax), prim.ctypes.data_as(A.u32p), _fptr(t), _fptr(b))
        return prim, t, b

    def trace_any(self, o, d, tmax):
        o, d, tmax = (np.ascontiguousarray(x, dtype=np.float32) for x in (o, d, tmax))
        n = len(tmax)
        hit = np.zeros(n, np.uint8)
        self._call("trace_any", self.h, n, _fptr(o), _fptr(d), _fptr(tmax), hit.ctypes.data_as(A.u8p))
        return hit


class Scene(Handle):
    """pt_scene handle + the render / parity entry points."""

    def __init__(self, lib, scene_data):
        self.L = lib
        super().__init__(lib.lib, lib.check, scene_data)

    @property
    def _ao(self):
        return self.L.ao   # the AO integrator's library, loaded on first use

    def _pass_size(self, name, *args, lib=None):
        s = C.c_uint32()
        self._call(name, self.h, *args, C.byref(s), lib=lib)
        return int(s.value)

    def pass_size(self, rp):
        """Samples per pixel per wavefront pass pt_render would use for `rp` now (the library's choice from the free memory when rp.spp_per_pass == 0)."""
        return self._pass_size("pass_size", C.byref(rp))

    def resolve_device(self, film_ptr, n_pixels, scale=1.0, rgb_ptr=None, srgb8_ptr=None):
        """pt_film_resolve_device: a film on the device -> rgb floats and / or 8-bit sRGB codes on the device (device pointers as integers)."""
        self._call("film_resolve_device", self.h, C.c_void_p(film_ptr), n_pixels, scale, C.c_void_p(rgb_ptr), C.c_void_p(srgb8_ptr))

    def halves_error(self, film_a_ptr, film_b_ptr, width, height, tile_error_ptr=None):
        """pt_film_halves_error of two half films on the device: (mean error, largest tile error); the per-tile errors go to `tile_error_ptr` when given."""
        mean, worst = C.c_float(), C.c_float()
        self._call("film_halves_error", self.h, C.c_void_p(film_a_ptr), C.c_void_p(film_b_ptr), width, height, C.c_void_p(tile_error_ptr), C.byref(mean), C.byref(worst))
        return mean.value, worst.value

    def render_progressive(self, rp, step, on_step=None, target_error=None):
        """The job `rp` in ranges of `step` samples, alternately into two torch films A and B on the device (A + B is the film). After each range:
        pt_film_halves_error of A and B, then on_step(done, mean_error, max_tile_error); nothing but those two numbers is read back. Stops when the job is done or,
        once both halves hold samples, when mean_error <= target_error. Returns (A + B as a numpy film (H, W, 4), samples rendered per pixel)."""
        if step <= 0:
            raise ValueError("step must be > 0")
        h, w = film_shape(rp)
        halves = _device_zeros((h, w, 4), (h, w, 4))
        done = k = 0
        while done < rp.spp:
            n = min(step, rp.spp - done)
            self.render(rp, device_ptr=halves[k % 2].data_ptr(), samples=(done, n))
            done += n; k += 1
            mean, worst = self.halves_error(halves[0].data_ptr(), halves[1].data_ptr(), w, h)
            if on_step is not None:
                on_step(done, mean, worst)
            if target_error is not None and k >= 2 and k % 2 == 0 and mean <= target_error:
                break
        return (halves[0] + halves[1]).cpu().numpy(), done

    def tile_grid(self, rp):
        """(ntx, nty) of the render's 16x16 sample-tile grid (pt_tile_grid): the grid rp.tile_rank / tile_world and the tile lists index, row major."""
        ntx, nty = C.c_uint32(), C.c_uint32()
        self._call("tile_grid", C.byref(rp), C.byref(ntx), C.byref(nty))
        return int(ntx.value), int(nty.value)

    def render_tiles(self, rp, samples, tiles, film=None, device_ptr=None):
        """pt_render_tiles: sample numbers samples = (first, n) of the listed tiles (strictly ascending indices into tile_grid(rp)) only, ADDED to `film`
        (a numpy film, made when None and returned) or to the device film at `device_ptr` (returns None)."""
        first, n = samples
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
        args = [self.h, C.byref(rp), first, n, tiles.ctypes.data_as(A.u32p), len(tiles)]
        return self._film_call("render_tiles", args, rp, film, device_ptr, None, self._lib)

    def select_tiles(self, rp, tile_error_ptr, threshold, candidates=None):
        """pt_tiles_select: of `candidates` (ascending tile indices; None: every tile of the grid) those whose film footprint meets a film tile whose error -- the
        device array pt_film_halves_error wrote, at `tile_error_ptr` -- is not <= threshold. A uint32 array, in the candidates' order."""
        if candidates is None:
            ntx, nty = self.tile_grid(rp)
            cand, n = None, ntx * nty
        else:
            candidates = np.ascontiguousarray(candidates, dtype=np.uint32)
            cand, n = candidates.ctypes.data_as(A.u32p), len(candidates)
        out = np.zeros(max(n, 1), dtype=np.uint32); n_out = C.c_uint32()
        self._call("tiles_select", self.h, C.byref(rp), C.c_void_p(tile_error_ptr), threshold, cand, n, out.ctypes.data_as(A.u32p), C.byref(n_out))
        return out[:n_out.value].copy()

    def render_adaptive(self, rp, threshold, step, min_samples=0, on_round=None):
        """The job `rp` with a shrinking set of active tiles: render_progressive's two half films, stopped tile by tile instead of as a whole frame.
        A round renders sample numbers [done, done + step) of the active tiles into film A and the next `step` into film B (both clipped to rp.spp). After a round in
        which both halves got samples, and once done >= min_samples, pt_film_halves_error writes the per-tile errors and pt_tiles_select keeps the active tiles whose
        footprint still meets a film tile with error > threshold. A tile that leaves the active set never returns, so all active tiles share one sample count and
        every call is one (first, n). Ends when no tile is active or done == rp.spp. on_round(done, active tiles, max_tile_error or None) is called after every round.
        Returns (A + B as a numpy film (H, W, 4), a (nty, ntx) uint32 array of the samples rendered per tile); self.adaptive_counters then holds the counters summed
        over the loop's render calls (counters() describes the last call alone).
        Caveat: the stopping rule reads the same samples it stops. A tile whose two halves happen to agree early stops early, so the estimate is biased (towards
        the values at which halves agree); min_samples bounds how early that can happen, it does not remove the bias."""
        if step <= 0:
            raise ValueError("step must be > 0")
        h, w = film_shape(rp)
        ntx, nty = self.tile_grid(rp)
        *halves, tile_err = _device_zeros((h, w, 4), (h, w, 4), (-(-w // 16)) * (-(-h // 16)))
        active = np.arange(ntx * nty, dtype=np.uint32)
        per_tile = np.zeros(ntx * nty, dtype=np.uint32)
        done, total = 0, None
        while done < rp.spp and len(active):
            got = []
            for half in halves:
                n = min(step, rp.spp - done)
                if n > 0:
                    self.render_tiles(rp, (done, n), active, device_ptr=half.data_ptr())
                    done += n; per_tile[active] += n
                    c = self.counters()
                    total = c if total is None else {k: ([a + x for a, x in zip(total[k], v)] if isinstance(v, list) else total[k] + v) for k, v in c.items()}
                got.append(n)
            worst = None
            if got[1] > 0 and done >= min_samples:
                _, worst = self.halves_error(halves[0].data_ptr(), halves[1].data_ptr(), w, h, tile_err.data_ptr())
                active = self.select_tiles(rp, tile_err.data_ptr(), threshold, candidates=active)
            if on_round is not None:
                on_round(done, active, worst)
        self.adaptive_counters = total
        return (halves[0] + halves[1]).cpu().numpy(), per_tile.reshape(nty, ntx)

    def render_aov(self, rp, samples=None, planes=AOV.PLANES, device_ptrs=None, sums=None):
        """The feature buffers of the job `rp` (pt_aov_render; `samples` = (first, n): pt_aov_render_samples): a dict of the un-normalised sums per wanted plane --
        "albedo" (H, W, 4) = sum w * rgb and sum w over all samples, "normal" (H, W, 4) = sum w * n and sum w over the samples that reach a surface, "depth" (H, W, 2) =
        sum w * t and the same weight. ADDED to the arrays of `sums` (a dict this method returned, for the same planes) when given, in place: a pixel's samples
        continue the chain of additions where the earlier call left it. `device_ptrs` = {plane: device pointer as an integer}: added to those buffers, returns None."""
        args = [self.h, C.byref(rp)] + ([] if samples is None else list(samples))
        name = "aov_render" if samples is None else "aov_render_samples"
        if device_ptrs is not None:
            self._call(name, *args, C.byref(AOV.buffers(device_ptrs, device=True)), 1, lib=self.L.aov); return None
        if sums is None:
            sums = {k: np.zeros(film_shape(rp) + (AOV.CHANNELS[k],), dtype=np.float32) for k in planes}
        self._call(name, *args, C.byref(AOV.buffers(sums)), 0, lib=self.L.aov)
        return sums

    def aov_pass_size(self, rp):
        """Samples per pixel per pass pt_aov_render would use for `rp` now."""
        return self._pass_size("aov_pass_size", C.byref(rp), lib=self.L.aov)

    def render_mattes(self, rp, layers=("material", "instance"), groups=None, samples=None, tables=None, device_ptrs=None):
        """The ID mattes of the job `rp` (pt_matte_render; `samples` = (first, n): pt_matte_render_samples): {layer: an (H, W) array of _abi_aov.MATTE_DTYPE} for the
        wanted layers of "material", "instance", "group" -- per pixel up to eight ids in first-seen order with the filter weight of their samples, w_total and
        w_other. `groups`: a uint32 array, the caller's id of every primitive (for per-shape mattes: the scene data's prim_group), needed by the "group" layer.
        `tables` (a dict this method returned, for the same layers) is CONTINUED in place: ranges rendered in ascending order leave what the whole range leaves, bit
        for bit. `device_ptrs` = {layer: device pointer as an integer}: those tables are continued, returns None."""
        args = [self.h, C.byref(rp)] + ([] if samples is None else list(samples))
        name = "matte_render" if samples is None else "matte_render_samples"
        groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)
        if device_ptrs is not None:
            self._call(name, *args, C.byref(AOV.matte_buffers(device_ptrs, groups, device=True)), 1, lib=self.L.aov); return None
        if tables is None:
            tables = {k: np.zeros(film_shape(rp), dtype=AOV.MATTE_DTYPE) for k in layers}
        self._call(name, *args, C.byref(AOV.matte_buffers(tables, groups)), 0, lib=self.L.aov)
        return tables

    def matte_pass_size(self, rp):
        """Samples per pixel per pass pt_matte_render would use for `rp` now."""
        return self._pass_size("matte_pass_size", C.byref(rp), lib=self.L.aov)

    def matte_mask(self, table, ids, n_pixels=None, mask_ptr=None):
        """pt_matte_mask: per pixel of one layer's table, the share of the filter weight that the ids of `ids` hold -- the matte of those materials, instances or
        groups, an (H, W) float32 array. `table`: an array of MATTE_DTYPE, or a device pointer as an integer to `n_pixels` tables (the result is then flat);
        `mask_ptr`: the mask goes to that device buffer, returns None."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        on_device = isinstance(table, int)
        if on_device:
            shape, tp = (n_pixels,), C.cast(C.c_void_p(table), AOV.mp)
        else:
            table = np.ascontiguousarray(table, dtype=AOV.MATTE_DTYPE)
            shape, tp = table.shape, table.ctypes.data_as(AOV.mp)
        n = int(np.prod(shape))
        if mask_ptr is not None:
            self._call("matte_mask", self.h, tp, int(on_device), n, ids.ctypes.data_as(A.u32p), len(ids), C.cast(C.c_void_p(mask_ptr), A.fp), 1, lib=self.L.aov); return None
        mask = np.zeros(shape, np.float32)
        self._call("matte_mask", self.h, tp, int(on_device), n, ids.ctypes.data_as(A.u32p), len(ids), _fptr(mask), 0, lib=self.L.aov)
        return mask

    def denoise(self, film_a, film_b, sums, params=None, device_ptrs=None):
        """pt_denoise of two half films (H, W, 4) -- XYZW sums of disjoint sample ranges, A + B is the film -- and the feature sums of the samples of A + B (the
        dict render_aov returns, all three planes): the denoised image (H, W, 3). `params`: a PtDenoiseParams, else the library's defaults.
        `device_ptrs` = (width, height, rgb_out): film_a, film_b, the values of `sums` and rgb_out are device pointers as integers; returns None."""
        lib = self.L.dn
        if params is None:
            params = default_denoise_params(self.L)
        if device_ptrs is not None:
            w, h, out = device_ptrs
            self._call("denoise", self.h, C.byref(params), C.c_void_p(film_a), C.c_void_p(film_b), C.byref(AOV.buffers(sums, device=True)), w, h, C.c_void_p(out), 1, lib=lib); return None
        film_a, film_b = (np.ascontiguousarray(f, dtype=np.float32) for f in (film_a, film_b))
        sums = {k: np.ascontiguousarray(sums[k], dtype=np.float32) for k in AOV.PLANES}
        h, w = film_a.shape[:2]
        for name, arr, ch in [("film_a", film_a, 4), ("film_b", film_b, 4)] + [(k, sums[k], AOV.CHANNELS[k]) for k in AOV.PLANES]:
            if arr.shape != (h, w, ch):
                raise ValueError(f"denoise: {name} has shape {arr.shape}, expected {(h, w, ch)}")
        out = np.zeros((h, w, 3), dtype=np.float32)
        self._call("denoise", self.h, C.byref(params), film_a.ctypes.data_as(C.c_void_p), film_b.ctypes.data_as(C.c_void_p), C.byref(AOV.buffers(sums)), w, h, out.ctypes.data_as(C.c_void_p), 0, lib=lib)
        return out

    def render_denoised(self, rp, params=None, inputs=False):
        """The job `rp` rendered and denoised without leaving the device: sample numbers [0, spp / 2) into half film A and [spp / 2, spp) into B (pt_render_samples),
        the feature sums of [0, spp) (pt_aov_render), pt_denoise of the three. Returns (the denoised image (H, W, 3), A + B as a numpy film (H, W, 4)); `inputs`: and (A, B, the feature sums) as the filter read them, numpy copies.
        counters() afterwards describes the feature render, kernel_stats() that render plus the denoiser's launches."""
        if rp.spp < 2:
            raise ValueError("render_denoised needs spp >= 2: two half films with samples in each")
        h, w = film_shape(rp)
        a, b, rgb, *features = _device_zeros((h, w, 4), (h, w, 4), (h, w, 3), *[(h, w, AOV.CHANNELS[k]) for k in AOV.PLANES])
        halves, planes = [a, b], dict(zip(AOV.PLANES, features))
        half = rp.spp // 2
        self.render(rp, device_ptr=halves[0].data_ptr(), samples=(0, half))
        self.render(rp, device_ptr=halves[1].data_ptr(), samples=(half, rp.spp - half))
        ptrs = {k: v.data_ptr() for k, v in planes.items()}
        self.render_aov(rp, device_ptrs=ptrs)
        self.denoise(halves[0].data_ptr(), halves[1].data_ptr(), ptrs, params, device_ptrs=(w, h, rgb.data_ptr()))
        out = (rgb.cpu().numpy(), (halves[0] + halves[1]).cpu().numpy())
        if inputs:
            out += ((halves[0].cpu().numpy(), halves[1].cpu().numpy(), {k: v.cpu().numpy() for k, v in planes.items()}),)
        return out

    def bake_select(self, select):
        """The prim_select bytes of pt_bake_*: `select` is a shape ordinal or a list of them -- resolved through the scene data's prim_group, the ordinal of every
        primitive's Shape call --, or a per-primitive array (bool or uint8, one entry per primitive) used as it is."""
        n = self.data.desc().n_prims
        if isinstance(select, np.ndarray) and select.dtype in (np.bool_, np.uint8):
            if select.shape != (n,):
                raise ValueError(f"bake: the selection has shape {select.shape}, the scene {n} primitives")
            return np.ascontiguousarray(select, dtype=np.uint8)
        ordinals = np.atleast_1d(np.asarray(select, dtype=np.int64))
        group = np.asarray(self.data.prim_group)
        return np.ascontiguousarray(np.isin(group, ordinals), dtype=np.uint8)

    def _bake_planes(self, kind, name, head, width, height, planes, samples, sums, device_ptrs):
        """What bake, bake_light and bake_transfer share: pt_<name> -- with `samples` = (first, n): pt_<name>_samples -- of the arguments `head` into the planes
        `planes` of BAKE.PLANE_TABLES[kind], each (H, W, channels) or, with one channel, (H, W). A plane `sums` does not hold yet starts from zeros; `device_ptrs` =
        {plane: device pointer as an integer}: the planes go to those buffers, returns None."""
        args = list(head) + ([] if samples is None else list(samples))
        name = name if samples is None else name + "_samples"
        struct = BAKE.BUFFERS[kind]
        if device_ptrs is not None:
            self._call(name, *args, C.byref(BAKE.buffers(device_ptrs, True, struct)), 1, lib=self.L.bake); return None
        if sums is None:
            sums = {}
        for k in planes:
            if k not in sums:
                channels, dtype = BAKE.PLANE_TABLES[kind][k]
                sums[k] = np.zeros((height, width) + ((channels,) if channels > 1 else ()), dtype=dtype)
        self._call(name, *args, C.byref(BAKE.buffers({k: sums[k] for k in planes}, False, struct)), 0, lib=self.L.bake)
        return sums

    def _bake_probe(self, name, head, queries, floats, light=False):
        """What the four *_rays methods share: pt_<name> of the arguments `head` for the queries named by the three index arrays `queries`. Returns a dict of the
        outputs: `floats` = ((key, is a 3-vector), ...) in the entry point's order, "found" (n,) uint8 and, with `light`, "light" (n,) uint32 ahead of them."""
        queries = [np.ascontiguousarray(v, dtype=np.uint32) for v in queries]
        n = len(queries[0])
        r = {k: np.zeros((n, 3) if vector else n, np.float32) for k, vector in floats}
        r["found"] = np.zeros(n, np.uint8)
        if light:
            r["light"] = np.zeros(n, np.uint32)
        self._call(name, *head, n, *[v.ctypes.data_as(A.u32p) for v in queries], *([r["light"].ctypes.data_as(A.u32p)] if light else []), *[_fptr(r[k]) for k, _ in floats],
                   r["found"].ctypes.data_as(A.u8p), lib=self.L.bake)
        return r

    def _light_selection(self, lights, nsamples):
        """((light_select pointer or None, n_lights) as pt_bake_light* and pt_bake_sh* take them, the light samples per sample: `nsamples`, None = one per selected light)"""
        lsel, n_lights, n_sel = self.bake_light_select(lights)
        return (None if lsel is None else lsel.ctypes.data_as(A.u8p), n_lights), n_sel if nsamples is None else nsamples

    def bake_params(self, width, height, spp, nsamples=64, cos_sample=True, max_distance=float("inf"), sampler="sobol", spp_per_pass=0, profile=False):
        return BAKE.PtBakeParams(width, height, spp, nsamples, 1 if cos_sample else 0, max_distance, _sampler_code(sampler), spp_per_pass, 1 if profile else 0)

    def bake(self, select, width, height, spp, nsamples=64, cos_sample=True, max_distance=float("inf"), sampler="sobol", samples=None, sums=None, device_ptrs=None,
             planes=BAKE.PLANES, spp_per_pass=0, profile=False):
        """pt_bake_render of the primitives `select` names (bake_select) into a width x height UV atlas (`samples` = (first, n): pt_bake_render_samples): a dict of
        the wanted planes -- "owner" (H, W) uint32, the primitive that owns the texel or PT_NONE; "position" and "normal" (H, W, 3); "ao_w" (H, W, 4) = the sums of
        the unoccluded AO directions and of their weights (resolve_bake turns them into the AO and bent-normal maps). owner, position and normal are written; ao_w
        is ADDED to the array of `sums` (a dict this method returned) when given, in place: sample ranges baked in ascending order leave what the whole range
        leaves. `device_ptrs` = {plane: device pointer as an integer}: the planes go to those buffers, returns None."""
        bp = self.bake_params(width, height, spp, nsamples, cos_sample, max_distance, sampler, spp_per_pass, profile)
        sel = self.bake_select(select)
        planes = tuple(planes) + tuple(k for k in (sums or {}) if k not in planes)   # (every plane `sums` holds is baked, as it always was)
        return self._bake_planes("bake", "bake_render", [self.h, C.byref(bp), sel.ctypes.data_as(A.u8p), len(sel)], width, height, planes, samples, sums, device_ptrs)

    def bake_pass_size(self, width, height, spp, nsamples=64, sampler="sobol", spp_per_pass=0):
        """Samples per texel per pass pt_bake_render would use now."""
        return self._pass_size("bake_pass_size", C.byref(self.bake_params(width, height, spp, nsamples, sampler=sampler, spp_per_pass=spp_per_pass)), lib=self.L.bake)

    def bake_dilate(self, owner, plane, iterations, device_ptrs=None):
        """pt_bake_dilate: the gutter round the islands of `plane` ((H, W) or (H, W, channels) float32) filled over `iterations` rings from the texels `owner`
        ((H, W) uint32, as Scene.bake returns it) covers; returns the dilated copy. `device_ptrs` = (width, height, channels): owner and plane are device
        pointers as integers, the plane is dilated in place, returns None."""
        if device_ptrs is not None:
            w, h, ch = device_ptrs
            self._call("bake_dilate", self.h, C.cast(C.c_void_p(owner), A.u32p), C.cast(C.c_void_p(plane), A.fp), ch, w, h, iterations, 1, lib=self.L.bake); return None
        owner = np.ascontiguousarray(owner, dtype=np.uint32)
        out = np.array(plane, dtype=np.float32, order="C")
        h, w = owner.shape
        ch = 1 if out.ndim == 2 else out.shape[2]
        if out.shape[:2] != (h, w):
            raise ValueError(f"bake_dilate: the plane has shape {out.shape}, the owner map {(h, w)}")
        self._call("bake_dilate", self.h, owner.ctypes.data_as(A.u32p), _fptr(out), ch, w, h, iterations, 0, lib=self.L.bake)
        return out

    def bake_rays(self, select, width, height, spp, texel, sample, element, nsamples=64, cos_sample=True, max_distance=float("inf"), sampler="sobol"):
        """pt_bake_rays: (origin (n, 3), direction (n, 3), weight (n,), found (n,) uint8) of the AO rays named by the arrays texel / sample / element."""
        bp = self.bake_params(width, height, spp, nsamples, cos_sample, max_distance, sampler)
        sel = self.bake_select(select)
        r = self._bake_probe("bake_rays", [self.h, C.byref(bp), sel.ctypes.data_as(A.u8p), len(sel)], (texel, sample, element), (("o", True), ("d", True), ("w", False)))
        return r["o"], r["d"], r["w"], r["found"]

    def bake_light_select(self, lights):
        """(light_select bytes or None, n_lights, n_sel) of pt_bake_light*: `lights` is None (all of the scene's lights), a list of light indices in the scene's
        light order, or a per-light array (bool or uint8, one entry per light) used as it is."""
        n = self.data.desc().n_lights
        if lights is None:
            return None, n, n
        if isinstance(lights, np.ndarray) and lights.dtype in (np.bool_, np.uint8):
            sel = np.ascontiguousarray(lights, dtype=np.uint8)
        else:
            sel = np.zeros(n, np.uint8)
            sel[np.atleast_1d(np.asarray(lights, dtype=np.int64))] = 1
        return sel, len(sel), int(np.count_nonzero(sel))

    def bake_light_params(self, width, height, spp, nsamples, sampler="sobol", spp_per_pass=0, profile=False):
        return BAKE.PtBakeLightParams(width, height, spp, nsamples, _sampler_code(sampler), spp_per_pass, 1 if profile else 0)

    def bake_light(self, select, width, height, spp, nsamples=None, lights=None, sampler="sobol", samples=None, sums=None, device_ptrs=None, planes=BAKE.LIGHT_PLANES,
                   spp_per_pass=0, profile=False):
        """pt_bake_light of the primitives `select` names (bake_select) under the lights `lights` names (bake_light_select; None: all) into a width x height UV atlas
        (`samples` = (first, n): pt_bake_light_samples): a dict of the wanted planes -- "owner", "position" and "normal" as Scene.bake, "light_w" (H, W, 4) = the sums
        of what the unoccluded light samples add and their count (resolve_lightmap turns them into the irradiance map). `nsamples` light samples per sample, None: one
        per selected light. light_w is ADDED to the array of `sums` as Scene.bake does. `device_ptrs` = {plane: device pointer}: returns None."""
        sel = self.bake_select(select)
        light_args, nsamples = self._light_selection(lights, nsamples)
        lp = self.bake_light_params(width, height, spp, nsamples, sampler, spp_per_pass, profile)
        return self._bake_planes("light", "bake_light", [self.h, C.byref(lp), sel.ctypes.data_as(A.u8p), len(sel), *light_args], width, height, planes, samples, sums, device_ptrs)

    def bake_light_pass_size(self, width, height, spp, nsamples=None, lights=None, sampler="sobol", spp_per_pass=0):
        """Samples per texel per pass pt_bake_light would use now."""
        light_args, nsamples = self._light_selection(lights, nsamples)
        return self._pass_size("bake_light_pass_size", C.byref(self.bake_light_params(width, height, spp, nsamples, sampler, spp_per_pass)), *light_args, lib=self.L.bake)

    def bake_light_rays(self, select, width, height, spp, texel, sample, element, nsamples=None, lights=None, sampler="sobol"):
        """pt_bake_light_rays: dict(light (n,) uint32, wi (n, 3), pdf (n,), Li (n, 3), E (n, 3), o (n, 3), d (n, 3), found (n,) uint8: bit 0 the texel has an owner,
        bit 1 the sample contributes and (o, d) is its shadow ray) of the light samples named by the arrays texel / sample / element."""
        sel = self.bake_select(select)
        light_args, nsamples = self._light_selection(lights, nsamples)
        lp = self.bake_light_params(width, height, spp, nsamples, sampler)
        return self._bake_probe("bake_light_rays", [self.h, C.byref(lp), sel.ctypes.data_as(A.u8p), len(sel), *light_args], (texel, sample, element), _LIGHT_SAMPLE, light=True)

    def bake_sh_params(self, points, spp, nsamples, sampler="sobol", row=None, spp_per_pass=0, profile=False):
        """(the points as a contiguous (n, 3) float32 array, the PtBakeShParams): `row` None = ceil(sqrt(n))."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(points)
        if row is None:
            row = max(1, math.isqrt(n))
            row += row * row < n
        return points, BAKE.PtBakeShParams(n, row, spp, nsamples, _sampler_code(sampler), spp_per_pass, 1 if profile else 0)

    def bake_sh(self, points, spp, nsamples=None, lights=None, sampler="sobol", row=None, samples=None, sums=None, device_ptr=None, spp_per_pass=0, profile=False):
        """pt_bake_sh: the direct light of the lights `lights` names (bake_light_select; None: all) at the free points `points` (n, 3), as sums over the nine order-2
        spherical harmonics (`samples` = (first, n): pt_bake_sh_samples). Returns sh_w (n, 28) = per point the 27 sums (coefficient q, channel c at 3 q + c) and the
        count of light samples that arrived (resolve_sh turns them into the coefficients, sh_irradiance evaluates those for a normal). `nsamples` light samples per
        sample, None: one per selected light. Point i is pixel (i mod row, i / row) of the sampler. The sums are ADDED to the array `sums` (what this method
        returned) when given, in place. `device_ptr`: sh_w is a device pointer as an integer, returns None."""
        light_args, nsamples = self._light_selection(lights, nsamples)
        points, hp = self.bake_sh_params(points, spp, nsamples, sampler, row, spp_per_pass, profile)
        args = [self.h, C.byref(hp), _fptr(points), *light_args] + ([] if samples is None else list(samples))
        name = "bake_sh" if samples is None else "bake_sh_samples"
        if device_ptr is not None:
            self._call(name, *args, C.cast(C.c_void_p(device_ptr), A.fp), 1, lib=self.L.bake); return None
        if sums is None:
            sums = np.zeros((len(points), BAKE.SH_SUMS), np.float32)
        if sums.shape != (len(points), BAKE.SH_SUMS) or sums.dtype != np.float32 or not sums.flags.c_contiguous:
            raise ValueError(f"bake_sh: sums must be a contiguous float32 array of shape {(len(points), BAKE.SH_SUMS)}")
        self._call(name, *args, _fptr(sums), 0, lib=self.L.bake)
        return sums

    def bake_sh_pass_size(self, n_points, spp, nsamples=None, lights=None, sampler="sobol", row=None, spp_per_pass=0):
        """Samples per point per pass pt_bake_sh would use now."""
        light_args, nsamples = self._light_selection(lights, nsamples)
        _, hp = self.bake_sh_params(np.zeros((n_points, 3), np.float32), spp, nsamples, sampler, row, spp_per_pass)
        return self._pass_size("bake_sh_pass_size", C.byref(hp), *light_args, lib=self.L.bake)

    def bake_sh_rays(self, points, spp, point, sample, element, nsamples=None, lights=None, sampler="sobol", row=None):
        """pt_bake_sh_rays: dict(light (n,) uint32, wi (n, 3), pdf (n,), Li (n, 3), E (n, 3), o (n, 3), d (n, 3), found (n,) uint8: bit 0 the point index is below
        the point count, bit 1 the sample contributes and (o, d) is its shadow ray) of the light samples named by the arrays point / sample / element."""
        light_args, nsamples = self._light_selection(lights, nsamples)
        points, hp = self.bake_sh_params(points, spp, nsamples, sampler, row)
        return self._bake_probe("bake_sh_rays", [self.h, C.byref(hp), _fptr(points), *light_args], (point, sample, element), _LIGHT_SAMPLE, light=True)

    def bake_transfer_params(self, width, height, front, back, spp=1, nsamples=64, cos_sample=True, max_distance=float("inf"), sampler="sobol", spp_per_pass=0, profile=False):
        return BAKE.PtBakeTransferParams(width, height, front, back, spp, nsamples, 1 if cos_sample else 0, max_distance, _sampler_code(sampler), spp_per_pass, 1 if profile else 0)

    def bake_transfer(self, source, select, width, height, front, back, spp=1, nsamples=64, cos_sample=True, max_distance=float("inf"), sampler="sobol", spp_per_pass=0, profile=False,
                      planes=BAKE.TRANSFER_PLANES, samples=None, sums=None, device_ptrs=None):
        """pt_bake_transfer: the Scene `source` projected onto the width x height UV atlas of this scene's primitives `select` names (bake_select), by rays from `front`
        above this scene's surface to `back` below it (`samples` = (first, n): pt_bake_transfer_samples). A dict of the wanted planes -- "owner" and "hit_prim" (H, W)
        uint32, "height" (H, W), "src_position", "src_normal" and "tangent_normal" (H, W, 3), "ao_w" (H, W, 4) = the AO sums at the source hit (resolve_bake) --, ADDED
        to the array of `sums` as Scene.bake does. Counters and kernel statistics of the call are `source`'s. `device_ptrs` = {plane: device pointer}: returns None."""
        tp = self.bake_transfer_params(width, height, front, back, spp, nsamples, cos_sample, max_distance, sampler, spp_per_pass, profile)
        sel = self.bake_select(select)
        return self._bake_planes("transfer", "bake_transfer", [self.h, source.h, C.byref(tp), sel.ctypes.data_as(A.u8p), len(sel)], width, height, planes, samples, sums, device_ptrs)

    def bake_transfer_pass_size(self, source, width, height, front, back, spp, nsamples=64, sampler="sobol", spp_per_pass=0):
        """AO samples per texel per pass pt_bake_transfer would use now."""
        tp = self.bake_transfer_params(width, height, front, back, spp, nsamples, sampler=sampler, spp_per_pass=spp_per_pass)
        return self._pass_size("bake_transfer_pass_size", source.h, C.byref(tp), lib=self.L.bake)

    def bake_transfer_rays(self, source, select, width, height, front, back, spp, texel, sample, element, nsamples=64, cos_sample=True, max_distance=float("inf"), sampler="sobol"):
        """pt_bake_transfer_rays: dict(o, d, t_max: the projection rays of the texels; ao_o, ao_d, ao_w: the AO rays (sample, element) from their detail hits; found (n,)
        uint8: bit 0 the texel has an owner, bit 1 a detail hit)."""
        tp = self.bake_transfer_params(width, height, front, back, spp, nsamples, cos_sample, max_distance, sampler)
        sel = self.bake_select(select)
        return self._bake_probe("bake_transfer_rays", [self.h, source.h, C.byref(tp), sel.ctypes.data_as(A.u8p), len(sel)], (texel, sample, element),
                                (("o", True), ("d", True), ("t_max", False), ("ao_o", True), ("ao_d", True), ("ao_w", False)))

    def ao_params(self):
        """The scene's PtAOParams (SceneBuilder.integ / the front end's "ambientocclusion" parameters)."""
        return self.data.ao_params()

    def ao_pass_size(self, rp, ao=None):
        """Samples per pixel per pass pt_ao_render would use for `rp` now."""
        return self._pass_size("ao_pass_size", C.byref(rp), C.byref(self.ao_params() if ao is None else ao), lib=self.L.ao)


class MultiScene(Handle):
    """pt_multi_scene: the scene replicated on several devices of THIS process (one host thread + stream per replica inside
    pt_multi_render); a device ordinal may repeat. The film comes back summed, on the first device or in a host array."""
    PREFIX = "pt_multi_"

    def __init__(self, lib, scene_data, devices):
        self.L = lib; self.devices = list(devices)
        devs = (C.c_int * len(self.devices))(*self.devices)
        super().__init__(lib.lib, lib.check, scene_data, devs, len(self.devices))

    def timing(self):
        """Last render: merge_ms and, per replica, the wall time of its pt_render and of its peer copy."""
        n = len(self.devices)
        merge = C.c_double(); r = (C.c_double * n)(); c = (C.c_double * n)()
        self._call("get_timing", self.h, C.byref(merge), r, c, n)
        return dict(merge_ms=merge.value, render_ms=list(r), copy_ms=list(c))

    def create_timing(self):
        """pt_multi_scene_create: wall time of the call and, per replica, of its own scene creation (replicas 1.. are created concurrently), in ms."""
        n = len(self.devices)
        wall = C.c_double(); r = (C.c_double * n)()
        self._call("get_create_timing", self.h, C.byref(wall), r, n)
        return dict(wall_ms=wall.value, replica_ms=list(r))

    def peer_access(self):
        """Per replica: "same device", "peer access" (device-to-device copies) or "staged through the host" -- how its film reaches the first device."""
        n = len(self.devices)
        p = (C.c_int * n)()
        self._call("get_peer_access", self.h, p, n)
        return [("same device", "peer access", "staged through the host")[v] for v in p]

    def kernel_stats(self, replica=0):
        return super().kernel_stats(replica)


def tile_shard(lib, rank, world, replica, n_replicas):
    r, w = C.c_uint32(), C.c_uint32()
    lib.lib.pt_multi_tile_shard(rank, world, replica, n_replicas, C.byref(r), C.byref(w))
    return r.value, w.value
