/* k_window_fast<14>: the last stage of wide batches, a tier whose layout lives in device memory (window_kernels.hpp, tier_pipeline.hpp: ID_LAST);
   in this unit alone the layout's pointers are global ones and the kernel asks for no LDS */
#define DACC_LAYOUT_IN_GLOBAL 1
#define DACC_INSTANTIATE_TIER 14
#include "window_kernels.hpp"
template __global__ void k_window_fast<14>(FastBatch, uint32_t const *, uint32_t *);
