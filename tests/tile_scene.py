"""Test infrastructure of the tile-list / adaptive-sampling tests (test_tile_grid.py, test_tile_lists.py, test_tiles_select.py, test_adaptive.py): render parameters under
another pixel filter, the two tile grids in numpy, and the scene whose left third is black background."""
import ctypes as C
import math

import numpy as np

F = np.float32


def with_filter(pkg, rp, kind, radius):
    """rp under the pixel filter `kind` of radius (r, r): table, radius and the sample / pixel bounds Film::get_sample_bounds derives from them (film.rs:104-112)."""
    r = float(radius)
    rp.filter_radius = (C.c_float * 2)(r, r)
    rp.filter_table = (C.c_float * 256)(*pkg.host.filter_table(kind, (r, r)))
    cb = rp.cropped_pixel_bounds
    sb = [math.floor(F(cb[0]) + F(0.5) - F(r)), math.floor(F(cb[1]) + F(0.5) - F(r)), math.ceil(F(cb[2]) - F(0.5) + F(r)), math.ceil(F(cb[3]) - F(0.5) + F(r))]
    rp.sample_bounds = (C.c_int32 * 4)(*sb)
    rp.pixel_bounds = (C.c_int32 * 4)(*sb)
    return rp


def grid_of(rp):
    """(ntx, nty) of the 16x16 tiles of rp.sample_bounds (integrator.rs:277-279)."""
    sb = rp.sample_bounds
    return -(-(sb[2] - sb[0]) // 16), -(-(sb[3] - sb[1]) // 16)


def footprint(rp, tile):
    """A sample tile's film footprint (x0, y0, x1, y1) as pt_tiles_select takes it: the pixels whose filter support overlaps the tile's area (Film::get_film_tile,
    film.rs:125-140, without the pixels whose support only touches the tile's edge), clipped to the crop; float32 with the kernel's floor / ceil."""
    sb, cb, (rx, ry) = rp.sample_bounds, rp.cropped_pixel_bounds, rp.filter_radius
    ntx, _ = grid_of(rp)
    tx0, ty0 = sb[0] + 16 * (tile % ntx), sb[1] + 16 * (tile // ntx)
    tx1, ty1 = min(tx0 + 16, sb[2]), min(ty0 + 16, sb[3])
    half = F(0.5)
    x0 = max(int(np.floor(F(F(tx0) - half) - F(rx))) + 1, cb[0]); y0 = max(int(np.floor(F(F(ty0) - half) - F(ry))) + 1, cb[1])
    x1 = min(int(np.ceil(F(F(tx1) - half) + F(rx))), cb[2]); y1 = min(int(np.ceil(F(F(ty1) - half) + F(ry))), cb[3])
    return x0, y0, x1, y1


def select_model(rp, tile_err, threshold, candidates=None):
    """pt_tiles_select in numpy: the candidates (None: every tile) whose footprint meets a film-grid tile f with not (tile_err[f] <= threshold), in order."""
    cb = rp.cropped_pixel_bounds
    fntx = -(-(cb[2] - cb[0]) // 16)
    ntx, nty = grid_of(rp)
    out = []
    for t in (range(ntx * nty) if candidates is None else candidates):
        x0, y0, x1, y1 = footprint(rp, int(t))
        if x0 >= x1 or y0 >= y1:
            continue
        fx0, fx1, fy0, fy1 = (x0 - cb[0]) // 16, (x1 - 1 - cb[0]) // 16, (y0 - cb[1]) // 16, (y1 - 1 - cb[1]) // 16
        e = np.asarray(tile_err, F).reshape(-1, fntx)[fy0:fy1 + 1, fx0:fx1 + 1]
        if (~(e <= F(threshold))).any():
            out.append(int(t))
    return np.array(out, np.uint32)


def tile_pixels(rp, tiles):
    """Boolean (H, W) mask over the cropped film of the pixels inside the listed sample tiles."""
    sb, cb = rp.sample_bounds, rp.cropped_pixel_bounds
    ntx, _ = grid_of(rp)
    mask = np.zeros((cb[3] - cb[1], cb[2] - cb[0]), bool)
    for t in tiles:
        x0, y0 = sb[0] + 16 * (int(t) % ntx), sb[1] + 16 * (int(t) // ntx)
        xa, ya, xb, yb = max(x0, cb[0]), max(y0, cb[1]), min(x0 + 16, sb[2], cb[2]), min(y0 + 16, sb[3], cb[3])
        if xa < xb and ya < yb:
            mask[ya - cb[1]:yb - cb[1], xa - cb[0]:xb - cb[0]] = True
    return mask


def background_scene(pkg, xres=48, yres=32, spp=16):
    """range_scene's content -- the area light, the noise-textured floor, the glass sphere -- moved to the right-hand two thirds of a 48x32 frame: the camera of
    range_scene looks along -z with image-left = world +x, and nothing of the scene reaches beyond x = 0.35, so the left 16 pixel columns see the black background only
    (no environment light: their radiance is exactly 0 in every sample)."""
    from range_scene import noise_image
    b = pkg.host.SceneBuilder()
    b.film.update(xres=xres, yres=yres); b.spp = spp; b.sampler = "sobol"
    b.integ.update(maxdepth=5, kind="path")
    b.look_at((0.0, 1.8, 6.0), (0.0, 0.2, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    b.attribute_begin(); b.area_light_source(L=(30.0, 28.0, 24.0))
    b.trianglemesh(np.array([(-3.0, 4.0, -1.0), (0.0, 4.0, -1.0), (-1.5, 4.0, 1.5)], np.float32), np.array([0, 1, 2], np.uint32)); b.attribute_end()
    b.texture("noise", "color", "imagemap", pixels=noise_image(), trilinear=True, uscale=12.0, vscale=12.0)
    b.material("matte", Kd="noise")
    P = np.array([(-8.0, -1.0, -8.0), (-8.0, -1.0, 8.0), (0.35, -1.0, 8.0), (0.35, -1.0, -8.0)], np.float32)
    b.trianglemesh(P, np.array([0, 1, 2, 0, 2, 3], np.uint32), UV=np.array([[0, 0], [0, 1], [1, 1], [1, 0]], np.float32))
    b.attribute_begin(); b.material("glass", Kr=(1.0, 1.0, 1.0), Kt=(1.0, 1.0, 1.0), eta=1.5); b.translate(-1.0, 0.0, 0.5); b.sphere(radius=1.0); b.attribute_end()
    sd, rp = b.world_end()
    rp.spp_per_pass = 4
    return sd, rp


BACKGROUND_PBRT = """LookAt 0 1.8 6  0 0.2 0  0 1 0
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" 48 "integer yresolution" 32 "string filename" "adaptive.pfm"
Sampler "sobol" "integer pixelsamples" 16
PixelFilter "box"
Integrator "path" "integer maxdepth" 5
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [30 28 24]
  Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 4 -1  0 4 -1  -1.5 4 1.5]
AttributeEnd
Texture "chk" "spectrum" "checkerboard" "float uscale" 40 "float vscale" 40 "rgb tex1" [0.9 0.9 0.9] "rgb tex2" [0.05 0.05 0.05]
Material "matte" "texture Kd" "chk"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-8 -1 -8  -8 -1 8  0.35 -1 8  0.35 -1 -8] "float st" [0 0 0 1 1 1 1 0]
AttributeBegin
  Material "glass"
  Translate -1 0 0.5
  Shape "sphere" "float radius" 1
AttributeEnd
WorldEnd
"""   # background_scene's layout as a scene file (a checkerboard for the noise image): the left 16 pixel columns see the black background only
