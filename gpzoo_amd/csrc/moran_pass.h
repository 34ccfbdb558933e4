// moran_pass.h -- Moran's I of the columns of an fp32 slab, for callers inside the library (residual.hip).  The kernels are
// narrow mi_rows / mi_final of spatial_stats.hip, which is built with fp contraction off; gpz_morans_i runs the same ones.
#pragma once
#include "common.h"

namespace gpz {

// bytes of scratch for a slab of B rows and up to `cols` columns
size_t moran_slab_bytes(int64_t B, int64_t cols);

// Columns 0 .. cols of slab (B rows of ld floats each, cols <= ld) over nbr (B, K): I, the column mean and the column
// variance sum z^2 / B, cols fp64 values each.  info[0] is set to 1 by a table entry outside [0, B) or naming its own row
// (it is not cleared here).  Every sum in a fixed order.
int moran_slab_run(const float* slab, int64_t B, int64_t cols, int64_t ld, const int64_t* nbr, int K, double* I, double* mean,
                   double* var, int32_t* info, void* scratch, hipStream_t s);

}  // namespace gpz
