/* k_window_fast<19>: the wide deep stage of wide batches (windows of 251 ... 1000 strings at w = 64 ... 127), a tier whose layout lives in device memory
   (window_kernels.hpp, tier_pipeline.hpp: ID_WDEEP); in this unit the layout's pointers are global ones and the kernel asks for no LDS */
#define DACC_LAYOUT_IN_GLOBAL 1
#define DACC_INSTANTIATE_TIER 19
#include "window_kernels.hpp"
template __global__ void k_window_fast<19>(FastBatch, uint32_t const *, uint32_t *);
