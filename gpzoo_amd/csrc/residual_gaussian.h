// residual_gaussian.h -- the residual pass of the Gaussian factor models (RSF, FA) for residual.hip, which includes this file
// after its own kernels and shares gene_of, for_ksteps, launch_slab, its plan and its driver with it; all that is host code
// here is gs_residual_slab, which names this family's kernels to launch_slab.  Residuals of real-valued expression under
//
//   yhat[d,n] = b[d] + sum_l W[d,l] mean[l,n]                  v[d,n] = sd[d]^2 + sum_l W[d,l]^2 scale[l,n]^2
//   kind 0, Pearson:     r = (y - yhat) / sd[d]
//   kind 1, response:    r =  y - yhat
//   kind 2, predictive:  r = (y - yhat) / sqrt(v)
//
// into the spot-major slab of residual.hip.  Dense y (D, B), or expression stored as the non-zeros z of its values minus a
// per-gene fp64 offset c: y = (float)((double)z - c), (float)(-c) where nothing is stored -- element for element the array
// SparseExpression.to_dense() holds.  The factor means are read where they are (no exponential, no copy); only the
// predictive kind needs an array of its own, scale^2 (Lt, B), in the plan's factor scratch.
//
//   gs_factors_kernel   scale^2 (Lt, B), predictive kind only
//   gs_tile_kernel      the geometry of rs_tile_kernel: grid (gene blocks of 64, spot slices), 4 waves, a 64-spot x 16-gene
//                       tile per wave on v_mfma_f32_16x16x4_f32 with the spots as rows, a lane holding 16 spots of ONE gene, y
//                       read once as 16-byte loads where the rows are aligned, stores straight from the registers in whole
//                       64-byte segments, columns beyond the slab's genes written as 0.  PRED adds a second accumulator chain,
//                       W^2 (squared once into registers) against scale^2; its A operands double, so the next tile's A
//                       operands are prefetched into registers up to KS = 4 there (KS = 8 without): the same 64 registers.
//                       Above KS = 10 the two A operands of a whole tile no longer fit beside the rest (SPLIT): they are
//                       loaded and multiplied one 16-spot sub-tile at a time.  No instance uses scratch memory.
//                       ZERO reads no y: every element gets the residual at y = (float)(-c[d]), launch 1 of the sparse entry.
//   gs_stored_kernel    launch 2 of the sparse entry, the scheme of rs_stored_kernel: one wave per chunk of at most 512 stored
//                       entries of a gene row, yhat (and v) formed again at the entry's spot BY THE SAME MFMA chain, so a
//                       stored entry gets the dense entry's bits; the residual overwrites the slab's element.
//
// One element-wise function, gs_residual, serves all three; residual.hip is built with fp contraction off, so it gives the
// same bits wherever it is inlined.  The division and the square root are the correctly rounded ones.
#pragma once

namespace gpz {
namespace rsd {

struct GArgs {
  const float *mean, *W, *b, *sd, *y;
  const double* offset;           // sparse expression: y = values - offset
  const int32_t* genes;
  grk::GrRows rows;
  const float* s2;                // (Lt, B) scale^2, predictive kind
  float* out;
  int64_t B, D, g0, ng, ld;
  int Lt, SN, kind;
};

// z = sum_l W m, z2 = sum_l W^2 s^2 (read by the predictive kind alone)
__device__ __forceinline__ float gs_residual(float y, float b, float z, float sd, float z2, int kind) {
  const float e = y - (b + z);
  if (kind == 1) return e;
  if (kind == 0) return e / sd;
  return e / sqrtf(sd * sd + z2);
}

__global__ __launch_bounds__(256) void gs_factors_kernel(const float* scale, float* s2, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float s = scale[i];
    s2[i] = s * s;
  }
}

template <int KS, bool PRED, bool ZERO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void gs_tile_kernel(GArgs a) {
  constexpr bool PFA = KS <= (PRED ? 4 : 8);    // the A operands of the next tile fit in registers beside the current ones
  constexpr bool SPLIT = PRED && KS > 10;       // both A operands of a whole tile do not fit: one 16-spot sub-tile at a time
  constexpr int KA = SPLIT ? 1 : KS;
  constexpr int KP = PRED ? KS : 1;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t col = ((int64_t)blockIdx.x * 4 + wave) * TG + r;   // this lane's column of the slab
  const int64_t gene = gene_of(a, col);
  const bool dok = gene >= 0, cok = col < a.ld;
  const int64_t ntiles = (a.B + TS - 1) / TS, tper = (ntiles + a.SN - 1) / a.SN;
  const int64_t t_lo = blockIdx.y * tper, t_hi = (t_lo + tper < ntiles) ? t_lo + tper : ntiles;
  const bool vec = !ZERO && (a.B & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;   // rows of y start 16-byte aligned
  const float bd = dok ? a.b[gene] : 0.f, sd = dok ? a.sd[gene] : 1.f;
  const float y0 = (ZERO && dok) ? (float)(-a.offset[gene]) : 0.f;
  float wb[KS], w2[SPLIT ? 1 : KP];             // B[k = factor 4 ks + q][column r], and its square (SPLIT: squared at its use)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = (dok && l < a.Lt) ? a.W[gene * a.Lt + l] : 0.f;
    if (PRED && !SPLIT) w2[ks] = wb[ks] * wb[ks];
  }
  const int arow = 16 * (r >> 2) + (r & 3);     // A row r of sub-tile c is spot 16 (r >> 2) + 4c + (r & 3) of the tile
  struct Tile { f4 yv[4]; float av[4][KA], sv[4][SPLIT ? 1 : KP]; };
  auto load_tile = [&](int64_t tt, Tile& T) __attribute__((always_inline)) {
    const int64_t n0 = tt * TS;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t n = n0 + 16 * q + 4 * c;
      T.yv[c] = f4{y0, y0, y0, y0};
      if (!ZERO && dok) {
        const float* yp = a.y + gene * a.B + n;
        if (vec && n + 3 < a.B) T.yv[c] = *reinterpret_cast<const f4*>(yp);
        else {
#pragma unroll
          for (int g = 0; g < 4; ++g) if (n + g < a.B) T.yv[c][g] = yp[g];
        }
      }
    }
  };
  // factor 4 ks + q at spot nu + arow: one pointer per lane, every other term of the address is wave-uniform
  const float *mq = a.mean + (int64_t)q * a.B + arow, *sq = PRED ? a.s2 + (int64_t)q * a.B + arow : nullptr;
  auto load_sub = [&](int64_t nu, int64_t rowB, float* av, float* sv) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bool ok = 4 * ks + q < a.Lt && nu + arow < a.B;
      const int64_t u = (int64_t)(4 * ks) * rowB + nu;
      av[ks] = ok ? mq[u] : 0.f;
      if (PRED) sv[ks] = ok ? sq[u] : 0.f;
    }
  };
  auto load_a = [&](int64_t tt, Tile& T) __attribute__((always_inline)) {
    if (SPLIT) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) load_sub(tt * TS + 4 * c, a.B, T.av[c], T.sv[c]);
  };
  Tile cur, nxt;
  if (!SPLIT && t_lo < t_hi) { load_tile(t_lo, cur); if (PFA) load_a(t_lo, cur); }
  nxt = cur;
  for (int64_t tt = t_lo; tt < t_hi; ++tt) {
    const int64_t n0 = tt * TS;
    if (SPLIT) load_tile(tt, cur);              // y is not needed before the epilogue: the four sub-tiles cover its latency
    else {
      if (!PFA) load_a(tt, cur);
      if (tt + 1 < t_hi) { load_tile(tt + 1, nxt); if (PFA) load_a(tt + 1, nxt); }
    }
    // row 4q + g of sub-tile c is spot 16q + 4c + g, column r is this lane's gene
    f4 z[4], z2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float av1[KS], sv1[KP];
      if (SPLIT) {
        // the loads of one sub-tile stay behind the products of the one before, and the row stride is opaque here, or the
        // 2 KS row pointers are formed once before the loop and held in 4 KS registers
        __builtin_amdgcn_sched_barrier(0);
        int64_t rowB = a.B;
        asm volatile("" : "+s"(rowB));
        load_sub(n0 + 4 * c, rowB, av1, sv1);
      }
      const float *av = SPLIT ? av1 : cur.av[c], *sv = SPLIT ? sv1 : cur.sv[c];
      z[c] = f4{0, 0, 0, 0};
      z2[c] = f4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        z[c] = mfma4(av[ks], wb[ks], z[c]);
        if (PRED) z2[c] = mfma4(sv[ks], SPLIT ? wb[ks] * wb[ks] : w2[SPLIT ? 0 : ks], z2[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t n = n0 + 16 * q + 4 * c + g;
        if (cok && n < a.B) {
          const float res = gs_residual(cur.yv[c][g], bd, z[c][g], sd, z2[c][g], PRED ? 2 : a.kind);
          a.out[n * a.ld + col] = dok ? res : 0.f;
        }
      }
    if (!SPLIT) cur = nxt;
  }
}

// grid (slab columns, ceil(ceil(B / CHUNK) / 4)), 4 waves: wave = one chunk of the column's gene row
template <int KS, bool PRED>
__global__ __launch_bounds__(256) void gs_stored_kernel(GArgs a) {
  constexpr int KP = PRED ? KS : 1;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t col = blockIdx.x;
  const int64_t gene = gene_of(a, col);
  if (gene < 0) return;
  int64_t lo, hi;
  grk::gr_row(a.rows, gene, lo, hi);
  const int64_t p0 = lo + ((int64_t)blockIdx.y * 4 + wave) * CHUNK;
  if (p0 >= hi) return;                         // wave-uniform
  const int64_t p1 = p0 + CHUNK < hi ? p0 + CHUNK : hi;
  const float bd = a.b[gene], sd = a.sd[gene];
  const double off = a.offset[gene];
  float wb[KS], w2[KP];                         // B[k = factor 4 ks + q][every column]: the gene's W, and its square
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + q;
    wb[ks] = l < a.Lt ? a.W[gene * a.Lt + l] : 0.f;
    if (PRED) w2[ks] = wb[ks] * wb[ks];
  }
  // A row i of sub-tile c is entry 16c + i of the 64; the lane's outputs are rows 4q + g, so it finishes entry
  // 16 (r >> 2) + 4q + (r & 3), taken from sub-tile r >> 2, register r & 3
  const int mine = 16 * (r >> 2) + 4 * q + (r & 3);
  for (int64_t pb = p0; pb < p1; pb += 64) {    // wave-uniform trip count: every lane reaches every MFMA
    const int64_t p = pb + lane;
    int32_t spot = -1;
    float y = 0.f;
    if (p < p1) {
      int32_t sp;
      float x;
      if (grk::gr_entry(a.rows, p, sp, x)) { spot = sp; y = (float)((double)x - off); }
    }
    f4 z[4], z2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int32_t sa = __shfl(spot, 16 * c + r);
      z[c] = f4{0, 0, 0, 0};
      z2[c] = f4{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int l = 4 * ks + q;
        const bool ok = l < a.Lt && sa >= 0;
        z[c] = mfma4(ok ? a.mean[(int64_t)l * a.B + sa] : 0.f, wb[ks], z[c]);
        if (PRED) z2[c] = mfma4(ok ? a.s2[(int64_t)l * a.B + sa] : 0.f, w2[ks], z2[c]);
      }
    }
    const int32_t ms = __shfl(spot, mine);
    const float my = __shfl(y, mine);
    float zz = 0.f, zz2 = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        zz = (4 * c + g == r) ? z[c][g] : zz;
        zz2 = (4 * c + g == r) ? z2[c][g] : zz2;
      }
    if (ms >= 0) a.out[(int64_t)ms * a.ld + col] = gs_residual(my, bd, zz, sd, zz2, PRED ? 2 : a.kind);
  }
}

// the residual pass of one slab (launch_slab of residual.hip): the predictive kind has instances of its own
static int gs_residual_slab(const GArgs& a, bool sparse, hipStream_t s) {
  return for_ksteps(a.Lt, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    if (a.kind == 2)
      return launch_slab(gs_tile_kernel<KS, true, false>, gs_tile_kernel<KS, true, true>, gs_stored_kernel<KS, true>, a, sparse, s);
    return launch_slab(gs_tile_kernel<KS, false, false>, gs_tile_kernel<KS, false, true>, gs_stored_kernel<KS, false>, a, sparse, s);
  });
}

}  // namespace rsd
}  // namespace gpz
