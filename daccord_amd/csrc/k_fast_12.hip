/* k_window_fast<12>: one LDS tier of the window kernel per translation unit (window_kernels.hpp) */
#define DACC_INSTANTIATE_TIER 12
#include "window_kernels.hpp"
template __global__ void k_window_fast<12>(FastBatch, uint32_t const *, uint32_t *);
