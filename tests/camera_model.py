"""Test infrastructure of the camera tests (test_cameras_host.py, test_cameras.py): the numpy side of the three cameras.

The oracle renders the perspective camera only, so the orthographic and the environment camera have no oracle. Their tests follow aov_reference.py: a numpy model of
the camera (this file), proved where an oracle exists -- rays() of the perspective camera equals orc_camera_rays bit for bit -- and identities that hold the device
against the unchanged oracle's pieces: the model's rays -> orc_trace_closest give the primitive, t and barycentrics of every camera sample.

All arithmetic is tests/model_math.py's: float32 with nothing fused, as dev_math.h writes it, sine and cosine the oracle's orc_dm_sin / orc_dm_cos (the functions the
device uses), the camera samples the oracle's samplers'.

The reference's behaviours the model reproduces (cameras/orthographic.rs, cameras/environment.rs, core/camera.rs):
  * orthographic, lens: the differentials take ft from the ALREADY lens-modified direction's z (orthographic.rs:130), and the y focus point is
    pcamera + dy_camera + (0, 0, 0.1) * ft (:135) where x has (0, 0, 1). `corrected=True` gives the variant a well-meant fix would compute.
  * transform_ray moves the main ray's origin by its error bound, not the auxiliary origins (transform.rs:565-575); no direction is normalised after camera_to_world.
  * environment: theta = PI * pfilm.y / full_resolution.y, phi = 2 PI * pfilm.x / full_resolution.x over the FULL resolution; no differentials at all."""
import numpy as np
from model_math import F, PI, concentric_sample_disk, dm_cos, dm_sin, normalize, sampler_values, transform_ray, xf_point, xf_vector

PERSPECTIVE, ORTHOGRAPHIC, ENVIRONMENT = 0, 1, 2


def _camera_space(oracle, rp, cs, kind):
    """(pcamera, ray origin, ray direction, lens point or None) in camera space, before transform_ray."""
    N = len(cs)
    r2c = rp.raster_to_camera
    pfilm = np.stack([cs[:, 0], cs[:, 1], np.zeros(N, F)], 1).astype(F)
    pcamera = xf_point(r2c, pfilm)
    if kind == ORTHOGRAPHIC:   # orthographic.rs:104-106
        ro, rd = pcamera.copy(), np.tile(np.array([0.0, 0.0, 1.0], F), (N, 1))
    else:                      # perspective.rs:126-128
        ro, rd = np.zeros((N, 3), F), normalize(pcamera)
    plens = None
    if F(rp.lens_radius) > 0:  # perspective.rs:131-141, orthographic.rs:109-121
        dsk = concentric_sample_disk(oracle, cs[:, 3:5])
        plens = np.stack([dsk[:, 0] * F(rp.lens_radius), dsk[:, 1] * F(rp.lens_radius), np.zeros(N, F)], 1).astype(F)
        ft = (F(rp.focal_distance) / rd[:, 2]).astype(F)
        pfocus = (ro + (rd * ft[:, None]).astype(F)).astype(F)
        ro = plens
        rd = normalize((pfocus - ro).astype(F))
    return pcamera, ro, rd, plens


def rays(oracle, rp, cs):
    """The main ray of rp's camera for the camera samples cs (N, 5: pfilm.xy, time, plens.xy): (origins, directions), float32 (N, 3)."""
    cs = np.ascontiguousarray(cs, F)
    kind, N = rp.camera_type, len(cs)
    if kind == ENVIRONMENT:   # environment.rs:36-51
        theta = (PI * cs[:, 1] / F(rp.full_resolution[1])).astype(F)
        phi = (F(2.0) * PI * cs[:, 0] / F(rp.full_resolution[0])).astype(F)
        st, ct = dm_sin(oracle, theta), dm_cos(oracle, theta)
        sp, cp = dm_sin(oracle, phi), dm_cos(oracle, phi)
        ro, rd = np.zeros((N, 3), F), np.stack([st * cp, ct, st * sp], 1).astype(F)
    else:
        _, ro, rd, _ = _camera_space(oracle, rp, cs, kind)
    return transform_ray(rp.camera_to_world, ro, rd)


def dxdy_camera(rp):
    """dx_camera, dy_camera: perspective.rs:64-70 (differences of transformed points), orthographic.rs:55-56 (raster_to_camera on the vectors)."""
    r2c = rp.raster_to_camera
    e = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    if rp.camera_type == ORTHOGRAPHIC:
        v = xf_vector(r2c, e)
        return v[1], v[2]
    p = xf_point(r2c, e)
    return (p[1] - p[0]).astype(F), (p[2] - p[0]).astype(F)


def differentials(oracle, rp, cs, corrected=False):
    """What the shade kernels use: (out (N, 12): rx origin, rx direction, ry origin, ry direction after transform_ray and scale_differential(1 / sqrt(spp)), has (N,) uint8).
    corrected: the orthographic lens case with (0, 0, 1) for y as for x -- NOT what the reference computes; for the test that shows the quirk."""
    cs = np.ascontiguousarray(cs, F)
    kind, N = rp.camera_type, len(cs)
    if kind == ENVIRONMENT:   # core/camera.rs:43-97 writes into rd.diff only where generate_ray left one: it left None
        return np.zeros((N, 12), F), np.zeros(N, np.uint8)
    o, d = rays(oracle, rp, cs)
    pcamera, ro, rd, plens = _camera_space(oracle, rp, cs, kind)
    dxc, dyc = dxdy_camera(rp)
    if kind == ORTHOGRAPHIC:
        if plens is not None:   # orthographic.rs:126-138
            ft = (F(rp.focal_distance) / rd[:, 2]).astype(F)   # rd: the lens-modified direction (:130)
            zx = np.array([0.0, 0.0, 1.0], F)
            zy = zx if corrected else np.array([0.0, 0.0, 0.1], F)   # :135, as written there
            pfx = ((pcamera + dxc).astype(F) + (zx[None, :] * ft[:, None]).astype(F)).astype(F)
            pfy = ((pcamera + dyc).astype(F) + (zy[None, :] * ft[:, None]).astype(F)).astype(F)
            rx_o, ry_o = plens, plens
            rx_d, ry_d = normalize((pfx - plens).astype(F)), normalize((pfy - plens).astype(F))
        else:                   # orthographic.rs:140-143
            rx_o, ry_o = (pcamera + dxc).astype(F), (pcamera + dyc).astype(F)
            rx_d = ry_d = np.tile(np.array([0.0, 0.0, 1.0], F), (N, 1))
    elif plens is not None:     # perspective.rs:143-166
        dx = normalize((pcamera + dxc).astype(F))
        pfocus = (dx * (F(rp.focal_distance) / dx[:, 2]).astype(F)[:, None]).astype(F)
        rx_o, rx_d = plens, normalize((pfocus - plens).astype(F))
        dy = normalize((pcamera + dyc).astype(F))
        pfocus = (dy * (F(rp.focal_distance) / dy[:, 2]).astype(F)[:, None]).astype(F)
        ry_o, ry_d = plens, normalize((pfocus - plens).astype(F))
    else:                       # perspective.rs:167-172
        rx_o = ry_o = np.zeros((N, 3), F)
        rx_d, ry_d = normalize((pcamera + dxc).astype(F)), normalize((pcamera + dyc).astype(F))
    c2w = rp.camera_to_world
    sc = F(1.0) / np.sqrt(F(rp.spp))
    scale = lambda main, aux: (main + ((aux - main).astype(F) * sc).astype(F)).astype(F)   # ray.rs:34-41
    out = np.concatenate([scale(o, xf_point(c2w, rx_o)), scale(d, xf_vector(c2w, rx_d)), scale(o, xf_point(c2w, ry_o)), scale(d, xf_vector(c2w, ry_d))], 1)
    return np.ascontiguousarray(out, F), np.ones(N, np.uint8)


def camera_samples(pkg, oracle, rp, first=0, n=None):
    """(pix (N, 2) int32, cs (N, 5)) of the camera samples [first, first + n) of every pixel of rp's sample bounds, pixel major and sample minor, from the oracle's
    orc_sobol_samples / orc_halton_samples: get_camera_sample's p_film = pixel + get_2d(), time, p_lens (sampler.rs:170-180)."""
    n = rp.spp - first if n is None else n
    sb = rp.sample_bounds
    xs, ys = np.meshgrid(np.arange(sb[0], sb[2]), np.arange(sb[1], sb[3]), indexing="xy")
    pix = np.ascontiguousarray(np.repeat(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32), n, axis=0))
    sn = np.tile(np.arange(first, first + n, dtype=np.uint32), len(pix) // n)
    cs = sampler_values(oracle, pkg, rp.sampler_type, sb, pix, sn, 5, rp.sample_at_pixel_center)
    cs[:, :2] = pix.astype(F) + cs[:, :2]
    return pix, cs


def camera_hits(pkg, oracle, orc, rp, first=0, n=None, ray_source=None):
    """The camera samples [first, first + n) of every pixel of rp's sample bounds and their first hits by orc_trace_closest: dict(pix (N, 2), pfilm (N, 2), cs (N, 5),
    o, d (N, 3), prim, t, b, n), pixel major and sample minor. `orc`: the oracle's scene. ray_source(oracle, rp, cs) -> (o, d): where the rays come from -- the
    model's rays (the default) or aov_reference.oracle_rays (orc_camera_rays: the perspective camera's)."""
    pix, cs = camera_samples(pkg, oracle, rp, first, n)
    o, d = (ray_source or rays)(oracle, rp, cs)
    prim, t, b = orc.trace_closest(o, d, np.full(len(cs), np.inf, F))
    return dict(pix=pix, pfilm=cs[:, :2].copy(), cs=cs, o=o, d=d, prim=prim, t=t, b=b, n=rp.spp - first if n is None else n)


# ---- the jobs of the camera tests: 32 x 24 pixels x 4 samples under a box filter, a crop window that starts at (16, 4) of a 64 x 32 frame
XRES, YRES, CROP, SPP = 64, 32, (0.25, 0.75, 0.125, 0.875), 4


def job(pkg, kind, sampler="sobol", lens=False, spp=SPP, view="oblique", **camera_kw):
    """A builder with the film, the sampler and the camera set, after world_begin(). view "oblique": LookAt, Rotate and a non-uniform Scale in camera_to_world."""
    b = pkg.host.SceneBuilder()
    b.film.update(xres=XRES, yres=YRES, crop=CROP); b.spp = spp; b.sampler = sampler
    b.filter.update(kind="box", radius=(0.5, 0.5))
    if view == "oblique":
        b.scale(1.0, 1.25, 0.75); b.rotate(7.0, 0.2, 0.1, 1.0); b.look_at((0.3, 2.5, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    elif view == "down":   # straight down on the ground from y = 5, +x to the right and +z down the image
        b.look_at((0.0, 5.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    elif view == "shifted":   # a Scale and a Translate: matrices both hosts form without a rounding, for the byte comparisons
        b.scale(1.0, 1.25, 0.75); b.translate(0.5, -1.0, -6.0)
    kw = dict(camera_kw)
    if lens:
        kw.update(lensradius=0.05 if kind != "perspective" else 0.08, focaldistance=4.0 if kind != "perspective" else 6.5)
    if kind == "orthographic":
        kw.setdefault("screenwindow", (-4.0, 4.0, -1.5, 1.5))
    if kind == "perspective":
        kw.setdefault("fov", 40.0)
    b.camera(kind=kind, **kw)
    b.world_begin()
    return b


def film_corners(rp):
    """Camera samples at the four corners of the FULL resolution (for the environment camera theta = 0 and theta = pi, where sin(theta) is 0 or nearly 0)."""
    w, h = F(rp.full_resolution[0]), F(rp.full_resolution[1])
    return np.array([[0, 0, 0.5, 0.25, 0.75], [w, 0, 0.5, 0.25, 0.75], [0, h, 0.5, 0.75, 0.25], [w, h, 0.5, 0.5, 0.5]], F)
