// kernels_fast.hip -- the deform / frame / shared-morph kernels of kernels.hip once more, with multiply-add contraction allowed
// (models created with MMDX_CREATE_FAST_MATH): reached through kernels_fast() (kernels.hpp: kernel_set(true)).
// The library's default kernels stay uncontracted and bit-identical to the reference.
#define MMDX_FAST_MATH 1
#include "kernels.hip"
