/* k_window_fast<18>: the full-depth stage of shallow and deep batches (windows of 2001 ... 5001 strings and what tier 16 overflowed on), a tier whose layout
   lives in device memory (window_kernels.hpp, tier_pipeline.hpp: ID_FDEEP); in this unit the layout's pointers are global ones and the kernel asks for no LDS */
#define DACC_LAYOUT_IN_GLOBAL 1
#define DACC_INSTANTIATE_TIER 18
#include "window_kernels.hpp"
template __global__ void k_window_fast<18>(FastBatch, uint32_t const *, uint32_t *);
