"""A float32 numpy model of the SH points' contract (include/mi355bake.h "SH points") on the model of the lightmap (tests/lightmap_reference.py, whose
sample_lights it calls). Light samples come from the oracle's Light::sample_li (orc_light_sample_li) with p_error = n = 0 -- a reference point without surface --, occlusion from its
any-hit query (orc_trace_any) with t_max = 1 - 1e-4. As there, the oracle's hook does not hand out the far end p1 of the visibility segment:
  * point and spot lights: p1 = the light's position; the shadow ray is (p, p1 - p);
  * triangle lights: Triangle::sample restated, the model's own wi held bit for bit against the oracle's, the whole ray by spawn_ray_to;
  * sphere, disk, distant and infinite lights: the device's ray (pt_bake_sh_rays) is taken over after two checks -- its origin is p bit for bit (with n = 0
    offset_ray_origin adds nothing), its direction deviates from wi by at most 4 x what the model's exact rays of a triangle light of the same scene show
    (lightmap_reference.py's yardstick, margin and reason).
The sums: 28 per point, E.c * Y_q(wi) at 3 q + c and the count at 27, in ascending (s, k)."""
import numpy as np
import bake_reference as M
import lightmap_reference as LM
from model_math import F

T_MAX = LM.T_MAX
A_BAND = (F(3.141593), F(2.094395), F(0.785398))   # Ramamoorthi and Hanrahan's cosine-lobe factors of orders 0, 1, 2
A_Q = np.array([A_BAND[0]] + [A_BAND[1]] * 3 + [A_BAND[2]] * 5, F)


def basis(w):
    """Y_0 .. Y_8 (m, 9) at the rows (x, y, z) of w (m, 3): contract step 6, float32, unfused."""
    w = np.asarray(w, F).reshape(-1, 3)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(all="ignore"):
        Y = [np.full(len(w), F(0.282095), F), F(0.488603) * y, F(0.488603) * z, F(0.488603) * x, F(1.092548) * (x * y), F(1.092548) * (y * z),
             F(0.315392) * ((F(3.0) * (z * z)) - F(1.0)), F(1.092548) * (x * z), F(0.546274) * ((x * x) - (y * y))]
    return np.stack(Y, axis=1).astype(F)


def default_row(n):
    """ceil(sqrt(n))."""
    r = max(1, int(np.floor(np.sqrt(n))))
    while r * r < n:
        r += 1
    return r


def light_samples(oracle, pkg, sd, points, spp, nsamples, lights=None, sampler="sobol", row=None, samples=None, orc_scene=None, device=None):
    """Contract steps 1 to 5 for every light sample of the points: what lightmap_reference.sample_lights returns, `point` its items, in the order of
    bake_reference.sample_list(range(n_points), ..). `device`: what Scene.bake_sh_rays returns for those samples; needed (and held) for the lights whose p1 the
    model cannot restate. Without it such a light's ray goes from p along wi, 2 x rough_world_radius long, and is never compared with the device."""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n_points = len(points)
    row = default_row(n_points) if row is None else row
    rows = (n_points + row - 1) // row
    sel = LM.selected_lights(int(sd.desc().n_lights), lights)
    assert len(sel) > 0 and (spp * nsamples) % len(sel) == 0 and np.isfinite(points).all()
    pt, s, k = M.sample_list(np.arange(n_points), spp, nsamples, samples)
    u = M.array_samples(oracle, pkg, sampler, row, rows, pt % row, pt // row, s * nsamples + k)
    zero = np.zeros((len(pt), 3), F)   # the reference point {p, 0, 0}
    return LM.sample_lights(oracle, pkg, sd, "point", pt, s, k, u, points[pt], zero, zero, None, sel, nsamples, orc_scene or oracle.scene(sd), device)


def bake(oracle, pkg, sd, points, spp, nsamples=None, lights=None, sampler="sobol", row=None, samples=None, sh_w=None, orc_scene=None, device=None):
    """The model's bake: dict(sh_w (n, 28), n_rays, samples, occluded, nsamples). `device`: see light_samples."""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n_sel = len(LM.selected_lights(int(sd.desc().n_lights), lights))
    nsamples = n_sel if nsamples is None else nsamples
    orc_scene = orc_scene or oracle.scene(sd)
    r = light_samples(oracle, pkg, sd, points, spp, nsamples, lights, sampler, row, samples, orc_scene, device)
    ok = r["contributes"]
    n_rays = int(ok.sum())
    occ = orc_scene.trace_any(r["o"][ok], r["d"][ok], np.full(n_rays, T_MAX, F)) if n_rays else np.zeros(0, np.uint8)
    sh_w = np.zeros((len(points), 28), F) if sh_w is None else sh_w
    # sh_w (n, 28) += (E.c * Y_q(wi) at 3 q + c, 1) of the unoccluded contributing samples
    with np.errstate(all="ignore"):
        add = (r["E"][:, None, :] * basis(r["wi"])[:, :, None]).astype(F).reshape(-1, 27)
    M.accumulate(sh_w, r["point"], r, nsamples, np.concatenate([add, np.ones((len(ok), 1), F)], axis=1), LM.arrived(r, occ))
    return dict(sh_w=sh_w, n_rays=n_rays, samples=r, occluded=np.asarray(occ), nsamples=nsamples)


def resolve(sh_w, spp, nsamples):
    """(sh (n, 9, 3), reached (n,)): pt_bake_sh_resolve."""
    sh, reached = LM.resolve(np.asarray(sh_w, F).reshape(-1, 28), spp, nsamples)
    return sh.reshape(-1, 9, 3), reached


def irradiance(sh, normals):
    """E (n, 3) of the coefficients sh (n, 9, 3) under the unit normals (n, 3): pt_bake_sh_irradiance -- the sum over q ascending, from 0, of (A_q * sh[q, c]) * Y_q."""
    sh = np.asarray(sh, F).reshape(-1, 9, 3)
    Y = basis(normals)
    e = np.zeros((len(sh), 3), F)
    with np.errstate(all="ignore"):
        for q in range(9):
            e = (e + ((A_Q[q] * sh[:, q, :]).astype(F) * Y[:, q, None]).astype(F)).astype(F)
    return e
