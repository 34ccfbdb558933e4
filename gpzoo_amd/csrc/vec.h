// vec.h -- the clang vector types and the two packed primitives of the count and factor kernels (poisson.hip, nb.hip,
// nb_sparse.hip, the sparse-row kernels of sparse_rows.h).
#pragma once
#include "common.h"

namespace gpz {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// one k-step of 4 of a 16 x 16 fp32 product (v_mfma_f32_16x16x4_f32) and one packed multiply-add (v_pk_fma_f32)
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x2 pkfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

}  // namespace gpz
