// tu_camera.hip -- the generate kernel of the orthographic and the environment camera (kern_camera.h), in a code object of its own.
#include "kern_camera.h"
template __global__ void k_generate_cam<PT_CAMERA_ORTHOGRAPHIC>(RenderConst, SobolTables, PathSoA, uint32_t *, uint32_t *, DevCounters *);
template __global__ void k_generate_cam<PT_CAMERA_ENVIRONMENT>(RenderConst, SobolTables, PathSoA, uint32_t *, uint32_t *, DevCounters *);
