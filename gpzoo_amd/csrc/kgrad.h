// kgrad.h -- the one declaration of the kernel-gradient contraction (kgrad.hip) that svgp.hip, vnngp.hip and mmops.hip
// launch.  KgradArgs is passed by value into the kernel: every translation unit has to see this layout.
#pragma once
#include "common.h"

namespace gpz {

struct KgradArgs {
  const void* Kbar; int64_t ld, stride;
  const void* Z; const void* X;
  const int64_t* gZ; const int64_t* gX;
  const void* sigma; const void* ell; const void* ga; const void* gr2;
  double gpow, scalar_scale;
  int64_t M, ncols, Mp;
  int d, G;
  double* acc;  // (L, Mp, 8): dz0..dz3, dsigma, dlengthscale, da_eff, unused
};

// acc[l][m][0..6] += the contraction of Kbar's row m with dk/d(z_m, sigma_l, lengthscale_l, a_l); scalars times scalar_scale
int kgrad_launch(int dtype, int kind, const KgradArgs& a, int L, hipStream_t s);

}  // namespace gpz
