/* mi355front_matte.h -- what libmi355front.so adds for ID mattes (include/mi355aov.h: pt_matte_render): a channel-list EXR writer that
 * also takes string attributes (a Cryptomatte file's layer names, hash, conversion and manifests), and the ordinal of the Shape
 * directive behind every primitive of a parsed scene (per-shape mattes: PtMatteBuffers::prim_group).
 *
 * Kept beside include/mi355front.h, not in it: that header's set of entry points is what the checkpoint and range tests pin, and
 * a host that writes no mattes needs neither function. */
#ifndef MI355FRONT_MATTE_H
#define MI355FRONT_MATTE_H
#include <stdint.h>
#include "mi355front.h"
#ifdef __cplusplus
extern "C" {
#endif
/* ptf_write_exr_channels (mi355front.h) plus n_attrs header attributes of type "string", written after the required attributes in the
 * order given: name, '\0', "string", '\0', the value's size in bytes, the value's bytes. With n_attrs == 0 the file is
 * ptf_write_exr_channels' byte for byte. A NULL or empty name, a name of more than 31 bytes (the file's version word promises short
 * names) or a NULL value: PT_ERR_INVALID_ARG, no file written. */
int ptf_write_exr_channels_attrs(const char *path, int width, int height, uint32_t n_channels, const char *const *names, const float *const *data, const uint32_t *strides,
                                 uint32_t n_attrs, const char *const *attr_names, const char *const *attr_values);
/* Per primitive of ptf_scene_desc(scene) -- n_prims entries, a view valid until ptf_scene_destroy -- the ordinal of the Shape
 * directive it came from: 0, 1, 2, ... in file order, shapes inside ObjectBegin / ObjectEnd counted like any other. */
int ptf_prim_shape_ordinals(const ptf_scene *scene, const uint32_t **ordinals, uint32_t *n_prims);
#ifdef __cplusplus
}
#endif
#endif
