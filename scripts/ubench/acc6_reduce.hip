// scripts/ubench/acc6_reduce.hip -- gl::Acc6::reduce compiled alone, for scripts/count_valu.py (six loads, the reduction, one store)
#include "gl.hpp"

extern "C" __global__ void acc6_reduce_alone(const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    gl::Acc6 acc;
#pragma unroll
    for (int j = 0; j < 6; j++) acc.a[j] = in[6 * i + j];
    out[i] = acc.reduce();
}
