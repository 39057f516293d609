/* k_window_fast<17>: the long string stage of wide batches (windows with a B string of 129 ... 255 bases, on the second stream in front of the generic
   engine), a tier whose layout lives in device memory (window_kernels.hpp, tier_pipeline.hpp: ID_LONG); in this unit the layout's pointers are global
   ones and the kernel asks for no LDS.  One slab per workgroup: the layout first, the weights, the spill image and the instance image behind it */
#define DACC_LAYOUT_IN_GLOBAL 1
#define DACC_INSTANTIATE_TIER 17
#include "window_kernels.hpp"
template __global__ void k_window_fast<17>(FastBatch, uint32_t const *, uint32_t *);
