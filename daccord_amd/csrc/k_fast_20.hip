/* k_window_fast<20>: the stage of a batch with w = 128 (every window of it, strings of up to 255 bases, three words per position mask, a consensus of up to
   192 symbols), a tier whose layout lives in device memory (window_kernels.hpp, tier_pipeline.hpp: ID_W128); in this unit the layout's pointers are global
   ones and the kernel asks for no LDS */
#define DACC_LAYOUT_IN_GLOBAL 1
#define DACC_INSTANTIATE_TIER 20
#include "window_kernels.hpp"
template __global__ void k_window_fast<20>(FastBatch, uint32_t const *, uint32_t *);
