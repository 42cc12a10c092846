/* mi355front.h -- C ABI of the .pbrt scene-file front end (libmi355front.so).
 *
 * Replaces, on the host side, what `pbrt_parse` + `API` do in the reference before `integ.render(&scene)`
 * (pbrtparser/pbrtparser.rs:26-87, core/api.rs): it turns a .pbrt file into the PtSceneDesc / PtRenderParams that
 * libmi355pt.so consumes. Pure host C++ (no GPU code, no dependency on libmi355pt.so): a Rust host would keep its own
 * parser and only use include/mi355pt.h; this library is for hosts that have none (the `mi355pbrt` command line tool).
 * Supported subset and the directives that are rejected: see pbrt-rust_amd/frontend/frontend.cpp header. */
#ifndef MI355FRONT_H
#define MI355FRONT_H
#include <stddef.h>
#include "mi355pt.h"
#include "mi355ao.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct ptf_scene ptf_scene;
/* Parse a scene file / an in-memory scene (file names resolve against base_dir). PT_OK or PT_ERR_INVALID_ARG + ptf_last_error(). */
int ptf_parse_file(const char *path, ptf_scene **out);
int ptf_parse_string(const char *text, const char *base_dir, ptf_scene **out);
const char *ptf_last_error(void);
/* Views into the parsed scene; valid until ptf_scene_destroy. */
const PtSceneDesc *ptf_scene_desc(const ptf_scene *scene);
const PtRenderParams *ptf_render_params(const ptf_scene *scene);
const char *ptf_output_filename(const ptf_scene *scene);   /* Film "string filename" */
/* The "ambientocclusion" parameters (nsamples, cossample; defaults 64, true) of a scene whose ptf_render_params reports
 * integrator == PT_INTEGRATOR_AO: render it with pt_ao_render (include/mi355ao.h). PT_OK or PT_ERR_INVALID_ARG. */
int ptf_ao_params(const ptf_scene *scene, PtAOParams *out);
void ptf_scene_destroy(ptf_scene *scene);
/* Film::write_image's PFM branch (core/imageio.rs:288-328): rgb = width*height*3 floats, top row first. */
int ptf_write_pfm(const char *path, int width, int height, const float *rgb);
/* write_image (core/imageio.rs:42-60): by extension -- exr (three FLOAT channels, uncompressed), png / tga (8-bit, gamma
 * encoded, imageio.rs:359-381), pfm. */
int ptf_write_image(const char *path, int width, int height, const float *rgb);
/* An EXR file of n_channels FLOAT channels (one part, scan lines, uncompressed): pixel (x, y) of channel i is data[i][(y * width + x) * strides[i]], top row
 * first. `names` in the byte-wise sorted order the format stores them in (e.g. "N.X" < "Z" < "albedo.B"); anything else is PT_ERR_INVALID_ARG. */
int ptf_write_exr_channels(const char *path, int width, int height, uint32_t n_channels, const char *const *names, const float *const *data, const uint32_t *strides);
/* read_image (core/imageio.rs:18-40): pfm, hdr, png, tga, exr (scan-line / tiled / multi-part, NO/RLE/ZIPS/ZIP). Call with rgb == NULL to get the
 * size, then with a buffer of width*height*3 floats (top row first). */
int ptf_read_image(const char *path, int *width, int *height, float *rgb, size_t capacity_floats);
/* Checkpoints of a render made in sample ranges (pt_render_samples; `mi355pbrt --checkpoint FILE`): the header below, then width * height * 4 floats, the raw XYZW
 * film sums of sample numbers [first_sample, first_sample + samples_done) of a job of `spp` samples per pixel. Little endian, as the host writes it. */
#define PTF_CHECKPOINT_MAGIC 0x4b433550u   /* "P5CK" */
typedef struct PtfCheckpointHeader {
    uint32_t magic, version;          /* PTF_CHECKPOINT_MAGIC, 1 */
    uint32_t width, height;           /* the cropped film */
    uint32_t spp;                     /* the job's samples per pixel */
    uint32_t first_sample;            /* where the render began */
    uint32_t samples_done;            /* samples per pixel in the film sums */
    uint32_t reserved;
    uint64_t params_hash;             /* ptf_params_hash of the job */
} PtfCheckpointHeader;
/* FNV-1a over the render parameters that decide the film: every byte of *params but spp_per_pass and profile (they change the schedule, not the result), and *ao when
 * given. */
uint64_t ptf_params_hash(const PtRenderParams *params, const PtAOParams *ao_or_null);
/* Writes header + film to `path` (through path + ".tmp" and a rename, so that a crash leaves the previous checkpoint). */
int ptf_checkpoint_write(const char *path, const PtfCheckpointHeader *header, const float *film_xyzw);
/* Reads the checkpoint at `path` for the job `expect` describes (samples_done is not compared). No such file: PT_OK, *samples_done = 0, film untouched. A file whose
 * magic, version, film size, spp, first_sample or params_hash differ, or that is truncated: PT_ERR_INVALID_ARG, ptf_last_error() names the field, film untouched. */
int ptf_checkpoint_read(const char *path, const PtfCheckpointHeader *expect, uint32_t *samples_done, float *film_xyzw);
#ifdef __cplusplus
}
#endif
#endif
