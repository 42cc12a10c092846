// tu_preview.hip -- the device film tools: resolve to rgb / 8-bit sRGB and the two-half-buffer convergence estimate.
#include "kern_preview.h"
