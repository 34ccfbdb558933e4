// gaussian_sparse.hip -- the Gaussian step of gaussian.hip for expression stored as its non-zeros minus a per-gene offset:
// y[d,n] = z[d,n] - c[d], where z (log1p of size-normalised counts) has exactly the sparsity of the counts and c is the
// per-gene centring.  The expected log-likelihood is quadratic in y, so the offset folds into the intercept and every
// output is an exact sum over the stored entries plus Lt x Lt Gram matrices; nothing of D x B elements is read, written
// or allocated.
//
// Batch of B spots, a[d] = b[d] + c[d], iv[d] = 1 / sd[d]^2, p[d,n] = a[d] + w_d . m_n, nz(d) / nz(n) the stored entries of
// gene d inside the batch / of batch spot n:
//   M1 = sum_n m_n (Lt)   G = sum_n m_n m_n^T (Lt,Lt)   S2[l] = sum_n s[l,n]^2   u = sum_d iv a w_d (Lt)   H = sum_d iv w_d w_d^T
//   sse[d]      = sum_nz(d) z (z - 2 p) + B a^2 + 2 a w_d . M1 + w_d^T G w_d          R[d] = sse[d] + sum_l w[d,l]^2 S2[l]
//   loglik      = sum_d [ -B (log sd[d] + log(2 pi) / 2) - iv R[d] / 2 ]
//   dmean[:,n]  = sum_nz(n) iv z w_d - u - H m_n            dscale[l,n] = -s[l,n] H[l,l]
//   dW[d,:]     = iv [ sum_nz(d) z m_n - a M1 - G w_d - S2 * w_d ]
//   db[d]       = iv [ sum_nz(d) z - B a - w_d . M1 ]       dsd[d] = -B / sd + R[d] / sd^3
//   ss[d]       = sum_nz(d) z^2 - (sum_nz(d) z)^2 / B       (the null sum of squares of R^2; the offset cancels)
// sse and R are differences of larger terms: the quadratic terms and every accumulation are fp64, only the dot product
// w_d . m_n inside p is formed in fp32.
//
// The entries arrive in the two orders of gpzoo_amd.likelihoods.SparseCounts (by spot: col_ptr, col_gene, col_val; by gene:
// row_ptr, row_spot, row_perm); a batch is a list of distinct spots (idx) with its inverse (pos, -1 outside the batch).
//
// Launches (no atomics, no workgroup waits on another, every sum in a fixed order -> two calls agree bit for bit; every
// workspace word that is read is written by the same call first):
//   gs_mt_kernel      mean transposed to [B][LT] (LT = Lt padded to the kernel instance, zeros beyond Lt): one spot's factors
//                     are one contiguous run
//   gs_wiv_kernel     iv[d] W[d,:] as [D][LT] for the spot pass (gradient calls only)
//   gs_s2_kernel      S2, one workgroup per factor
//   gs_gram_kernel    slabs of 256 rows: partial G and M1 over the spots, partial H and u over the genes (gradient calls only);
//                     gs_reduce_kernel adds the slabs in ascending order
//   chunks_kernel     the gene pass's work list: row d is cut into ceil(len_d / 512) chunks of consecutive entries
//   gs_spot_kernel    one wave per batch spot, lanes stride over the column's entries: dmean, dscale (gradient calls only)
//   gs_gene_kernel    one wave per (gene, chunk): partials of sum z m, sum z, sum z^2 and sum z (z - 2 p)
//   gs_finish_kernel  one wave per gene: chunk partials in chunk order, the quadratic forms; dW, db, dsd, sse, ss, loglik per gene
//   gs_total_kernel   the scalar
#include "common.h"
#include "mmops.h"
#include "sparse_rows.h"

namespace gpz {
namespace gsp {

constexpr int GS_MAXL = 64;      // factors
constexpr int GS_CHUNK = 512;    // entries of one gene row per wave of the gene pass
constexpr int GS_ROWS = 256;     // rows per slab of gs_gram_kernel
constexpr int GS_GENES = 16;     // genes per workgroup of gs_finish_kernel (4 per wave)

typedef float gf32x4 __attribute__((ext_vector_type(4)));

struct GsArgs {
  const float *mean, *scale, *W, *b, *sd;
  const double* offset;
  const int64_t* col_ptr; const int32_t* col_gene; const float* col_val;
  const int64_t* row_ptr; const int32_t* row_spot; const int32_t* row_perm;
  const int32_t *idx, *pos;
  float* mT;                     // [B][LT]
  float* wiv;                    // [D][LT]
  double *spart, *gpart;         // [nbS][GW], [nbG][GW] with GW = LT * LT + LT: the Gram matrix, then the vector
  double *ssum, *gsum;           // [GW]: G and M1; H and u
  double* S2;                    // [64]
  int32_t *cstart, *chunk_gene;  // [D + 1], [nchunks]
  double *partv, *parts;         // [nchunks][LT]: sum z m;  [nchunks][4]: sum z, sum z^2, sum z (z - 2 p), unused
  double* llg;                   // [D]
  double *loglik, *sse, *ss;
  float *dmean, *dscale, *dW, *db, *dsd;
  int64_t N, B, D, nnz, nchunks;
  int Lt, LT, nbS, nbG, grads;
};

static int gs_instance(int Lt) {
  const int sizes[] = {4, 8, 12, 16, 20, 24, 32, 40, 48, 64};
  for (int s : sizes) if (Lt <= s) return s;
  return 0;
}

__global__ __launch_bounds__(256) void gs_mt_kernel(GsArgs a) {
  __shared__ float xt[GS_MAXL][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * 64, j = j0 + lane;
  for (int l = wave; l < a.LT; l += 4) xt[l][lane] = (l < a.Lt && j < a.B) ? a.mean[(int64_t)l * a.B + j] : 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * a.LT; i += 256) {
    const int jj = i / a.LT, l = i - jj * a.LT;
    if (j0 + jj < a.B) a.mT[(j0 + jj) * a.LT + l] = xt[l][jj];
  }
}

__global__ __launch_bounds__(256) void gs_wiv_kernel(GsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.D * a.LT) return;
  const int64_t d = i / a.LT;
  const int l = (int)(i - d * a.LT);
  float v = 0.f;
  if (l < a.Lt) {
    const double sd = (double)a.sd[d];
    v = (float)((double)a.W[d * a.Lt + l] / (sd * sd));
  }
  a.wiv[i] = v;
}

// S2[l] = sum_n scale[l,n]^2 in fp64 and a fixed order: grid (64), factors beyond Lt get 0
__global__ __launch_bounds__(1024) void gs_s2_kernel(GsArgs a) {
  __shared__ double sh[16];
  const int l = blockIdx.x;
  double s = 0.0;
  if (l < a.Lt)
    for (int64_t n = threadIdx.x; n < a.B; n += 1024) {
      const double v = (double)a.scale[(int64_t)l * a.B + n];
      s += v * v;
    }
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) a.S2[l] = t;
}

// One slab of GS_ROWS rows: part[i * LT + j] = sum_r wt[r] x[r,i] x[r,j] and part[LT * LT + l] = sum_r at[r] x[r,l], rows ascending.
//   genes == 0: rows are the batch's spots, x = m_n, wt = at = 1            -> G and M1
//   genes == 1: rows are the genes, x = w_d, wt = iv[d], at = iv[d] a[d]    -> H and u
__global__ __launch_bounds__(256) void gs_gram_kernel(GsArgs a, int genes) {
  __shared__ float rt[64][GS_MAXL];
  __shared__ double wt[64], at[64], v1[4][64];
  const int tid = threadIdx.x, l = tid & 63, q = tid >> 6;
  const int LT = a.LT, LL = LT * LT;
  const int64_t R = genes ? a.D : a.B;
  const int64_t r0 = (int64_t)blockIdx.x * GS_ROWS, r1 = r0 + GS_ROWS < R ? r0 + GS_ROWS : R;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  double s1 = 0.0;
  for (int64_t t0 = r0; t0 < r1; t0 += 64) {
    const int nr = (int)(r1 - t0 < 64 ? r1 - t0 : 64);
    __syncthreads();                                   // the previous tile has been read
    for (int i = tid; i < 64 * LT; i += 256) {
      const int rr = i / LT, c = i - rr * LT;
      float v = 0.f;
      if (rr < nr) {
        const int64_t row = t0 + rr;
        v = genes ? (c < a.Lt ? a.W[row * a.Lt + c] : 0.f) : a.mT[row * LT + c];
      }
      rt[rr][c] = v;
    }
    if (tid < 64) {
      double w = 0.0, av = 0.0;
      if (tid < nr) {
        if (genes) {
          const double sd = (double)a.sd[t0 + tid];
          w = 1.0 / (sd * sd);
          av = w * ((double)a.b[t0 + tid] + a.offset[t0 + tid]);
        } else {
          w = av = 1.0;
        }
      }
      wt[tid] = w;
      at[tid] = av;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int e = tid + 256 * k;
      if (e < LL) {
        const int i = e / LT, j = e - i * LT;
        double s = acc[k];
        for (int r = 0; r < nr; ++r) s = fma(wt[r] * (double)rt[r][i], (double)rt[r][j], s);
        acc[k] = s;
      }
    }
    if (l < LT)
      for (int r = q; r < nr; r += 4) s1 = fma(at[r], (double)rt[r][l], s1);
  }
  double* part = (genes ? a.gpart : a.spart) + (int64_t)blockIdx.x * (LL + LT);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int e = tid + 256 * k;
    if (e < LL) part[e] = acc[k];
  }
  v1[q][l] = s1;
  __syncthreads();
  if (q == 0 && l < LT) part[LL + l] = (v1[0][l] + v1[1][l]) + (v1[2][l] + v1[3][l]);
}

// out[e] = sum_b part[b][e] in ascending b
__global__ __launch_bounds__(256) void gs_reduce_kernel(const double* part, int nb, int GW, double* out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= GW) return;
  double v = 0.0;
#pragma unroll 4
  for (int b = 0; b < nb; ++b) v += part[(int64_t)b * GW + e];
  out[e] = v;
}

// Spot pass.  4 waves per workgroup, wave = batch spot j (global spot n = idx[j]).  Each lane takes every 64th entry of the
// column, reads its gene's pre-scaled row iv W[d,:] and adds z iv W[d,l] to its fp64 partial of factor l.
template <int LT>
__global__ __launch_bounds__(256) void gs_spot_kernel(GsArgs a) {
  __shared__ double sH[LT * LT], su[LT];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < LT * LT; i += 256) sH[i] = a.gsum[i];
  if (threadIdx.x < LT) su[threadIdx.x] = a.gsum[LT * LT + threadIdx.x];
  __syncthreads();                 // the only barrier: a wave without a spot leaves after it
  const int64_t j = (int64_t)blockIdx.x * 4 + wave;
  if (j >= a.B) return;
  const int64_t n = a.idx ? a.idx[j] : j;
  const int64_t k0 = a.col_ptr[n], k1 = a.col_ptr[n + 1];
  double acc[LT];
#pragma unroll
  for (int l = 0; l < LT; ++l) acc[l] = 0.0;
  for (int64_t k = k0 + lane; k < k1; k += 64) {
    const double z = (double)a.col_val[k];
    const gf32x4* wr = reinterpret_cast<const gf32x4*>(a.wiv + (int64_t)a.col_gene[k] * LT);
#pragma unroll
    for (int l = 0; l < LT; l += 4) {
      const gf32x4 v = wr[l / 4];
      acc[l] = fma(z, (double)v[0], acc[l]); acc[l + 1] = fma(z, (double)v[1], acc[l + 1]);
      acc[l + 2] = fma(z, (double)v[2], acc[l + 2]); acc[l + 3] = fma(z, (double)v[3], acc[l + 3]);
    }
  }
  double mine = 0.0;
#pragma unroll
  for (int l = 0; l < LT; ++l) {
    const double t = wave_sum(acc[l]);
    if (lane == l) mine = t;
  }
  const int ll = lane < LT ? lane : 0;
  const float mym = lane < LT ? a.mT[j * LT + lane] : 0.f;
  double hm = 0.0;
  for (int c = 0; c < LT; ++c) hm = fma(sH[c * LT + ll], (double)__shfl(mym, c), hm);
  if (lane < a.Lt) {
    const int64_t o = (int64_t)lane * a.B + j;
    a.dmean[o] = (float)(mine - su[lane] - hm);
    a.dscale[o] = (float)(-(double)a.scale[o] * sH[lane * LT + lane]);
  }
}

// Gene pass.  4 waves per workgroup, wave = chunk w of the work list: at most 512 consecutive entries of one gene row.  The
// wave first packs the chunk's entries that lie in the batch (pos[n] >= 0) into LDS, in their order, then every lane takes
// every 64th packed entry: with a batch of a fifth of the spots four lanes in five would otherwise idle.
template <int LT>
__global__ __launch_bounds__(256) void gs_gene_kernel(GsArgs a) {
  __shared__ int32_t lj[4][GS_CHUNK];
  __shared__ float lz[4][GS_CHUNK];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wi = (int64_t)blockIdx.x * 4 + wave;
  const int g = wi < a.nchunks ? a.chunk_gene[wi] : -1;
  int cnt = 0;
  if (g >= 0) {
    const int64_t p0 = a.row_ptr[g] + (wi - a.cstart[g]) * GS_CHUNK;
    const int64_t pe = a.row_ptr[g + 1], p1 = p0 + GS_CHUNK < pe ? p0 + GS_CHUNK : pe;
    // spot -> batch column -> position in the by-spot order -> value is a chain of four dependent loads: the chunk's eight
    // chains per lane are issued level by level, so that eight loads are in flight instead of one
    constexpr int U = GS_CHUNK / 64;
    int32_t nn[U], jj[U], pp[U];
    float zz[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t p = p0 + u * 64 + lane;
      nn[u] = p < p1 ? a.row_spot[p] : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) jj[u] = nn[u] >= 0 ? (a.pos ? a.pos[nn[u]] : nn[u]) : -1;
#pragma unroll
    for (int u = 0; u < U; ++u) pp[u] = jj[u] >= 0 ? a.row_perm[p0 + u * 64 + lane] : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) zz[u] = jj[u] >= 0 ? a.col_val[pp[u]] : 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool keep = jj[u] >= 0;
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int at = cnt + __popcll(m & ((1ull << lane) - 1ull));
        lj[wave][at] = jj[u];
        lz[wave][at] = zz[u];
      }
      cnt += __popcll(m);
    }
  }
  __syncthreads();                 // every wave, with or without a chunk, arrives here exactly once
  if (g < 0) return;
  float w[LT];
#pragma unroll
  for (int l = 0; l < LT; ++l) w[l] = l < a.Lt ? a.W[(int64_t)g * a.Lt + l] : 0.f;
  const double ad = (double)a.b[g] + a.offset[g];
  double acc[LT];
#pragma unroll
  for (int l = 0; l < LT; ++l) acc[l] = 0.0;
  double sz = 0.0, szz = 0.0, sq = 0.0;
  for (int i = lane; i < cnt; i += 64) {
    const int64_t j = lj[wave][i];
    const double z = (double)lz[wave][i];
    const gf32x4* mp = reinterpret_cast<const gf32x4*>(a.mT + j * LT);
    float dot = 0.f;
#pragma unroll
    for (int l = 0; l < LT; l += 4) {
      const gf32x4 v = mp[l / 4];
      dot = __builtin_fmaf(w[l], v[0], dot); dot = __builtin_fmaf(w[l + 1], v[1], dot);
      dot = __builtin_fmaf(w[l + 2], v[2], dot); dot = __builtin_fmaf(w[l + 3], v[3], dot);
      if (a.grads) {
        acc[l] = fma(z, (double)v[0], acc[l]); acc[l + 1] = fma(z, (double)v[1], acc[l + 1]);
        acc[l + 2] = fma(z, (double)v[2], acc[l + 2]); acc[l + 3] = fma(z, (double)v[3], acc[l + 3]);
      }
    }
    const double p = ad + (double)dot;
    sz += z;
    szz = fma(z, z, szz);
    sq = fma(z, z - 2.0 * p, sq);
  }
  if (a.grads) {
    double mine = 0.0;
#pragma unroll
    for (int l = 0; l < LT; ++l) {
      const double t = wave_sum(acc[l]);
      if (lane == l) mine = t;
    }
    if (lane < LT) a.partv[wi * LT + lane] = mine;
  }
  sz = wave_sum(sz);
  szz = wave_sum(szz);
  sq = wave_sum(sq);
  if (lane == 0) {
    a.parts[wi * 4] = sz;
    a.parts[wi * 4 + 1] = szz;
    a.parts[wi * 4 + 2] = sq;
  }
}

// One wave per gene (4 genes per wave, one after the other); lane l holds factor l.
__global__ __launch_bounds__(256) void gs_finish_kernel(GsArgs a) {
  __shared__ double sG[GS_MAXL * GS_MAXL], sM1[GS_MAXL], sS2[GS_MAXL];
  const int LT = a.LT, LL = LT * LT;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < LL; i += 256) sG[i] = a.ssum[i];
  if (threadIdx.x < 64) {
    sM1[threadIdx.x] = (int)threadIdx.x < LT ? a.ssum[LL + threadIdx.x] : 0.0;
    sS2[threadIdx.x] = a.S2[threadIdx.x];
  }
  __syncthreads();
  const int ll = lane < LT ? lane : 0;
  const double Bd = (double)a.B;
  for (int q = 0; q < GS_GENES / 4; ++q) {
    const int64_t d = ((int64_t)blockIdx.x * 4 + wave) * (GS_GENES / 4) + q;
    if (d >= a.D) return;
    const float wf = lane < a.Lt ? a.W[d * a.Lt + lane] : 0.f;
    const double w = (double)wf;
    double Gw = 0.0;
    for (int c = 0; c < LT; ++c) Gw = fma(sG[c * LT + ll], (double)__shfl(wf, c), Gw);
    if (lane >= LT) Gw = 0.0;
    const double wM1 = wave_sum(w * sM1[lane]);
    const double wGw = wave_sum(w * Gw);
    const double wS2w = wave_sum(w * w * sS2[lane]);
    double zm = 0.0, sz = 0.0, szz = 0.0, sq = 0.0;
    const int c0 = a.cstart[d], c1 = a.cstart[d + 1];
    for (int c = c0; c < c1; ++c) {
      if (a.grads && lane < LT) zm += a.partv[(int64_t)c * LT + lane];
      sz += a.parts[(int64_t)c * 4];
      szz += a.parts[(int64_t)c * 4 + 1];
      sq += a.parts[(int64_t)c * 4 + 2];
    }
    const double sd = (double)a.sd[d], iv = 1.0 / (sd * sd);
    const double ad = (double)a.b[d] + a.offset[d];
    const double sse = sq + Bd * ad * ad + 2.0 * ad * wM1 + wGw;
    const double R = sse + wS2w;
    if (lane == 0) {
      if (a.sse) a.sse[d] = sse;
      if (a.ss) a.ss[d] = szz - sz * sz / Bd;
      a.llg[d] = -Bd * (0.91893853320467274178 + log(sd)) - 0.5 * iv * R;
      if (a.grads) {
        a.db[d] = (float)(iv * (sz - Bd * ad - wM1));
        a.dsd[d] = (float)(-Bd / sd + R * iv / sd);
      }
    }
    if (a.grads && lane < a.Lt) a.dW[d * a.Lt + lane] = (float)(iv * (zm - ad * sM1[lane] - Gw - sS2[lane] * w));
  }
}

__global__ __launch_bounds__(1024) void gs_total_kernel(GsArgs a) {
  __shared__ double sh[16];
  double v = 0.0;
  for (int64_t j = threadIdx.x; j < a.D; j += 1024) v += a.llg[j];
  const double t = block_sum(v, sh);
  if (threadIdx.x == 0) a.loglik[0] = t;
}

struct GsPlan { int LT, nbS, nbG; int64_t nchunks; size_t bytes; };

static GsPlan gs_plan(int64_t B, int64_t D, int Lt, int64_t nnz, GsArgs* a, void* ws) {
  GsPlan p;
  p.LT = gs_instance(Lt);
  p.nbS = (int)((B + GS_ROWS - 1) / GS_ROWS);
  p.nbG = (int)((D + GS_ROWS - 1) / GS_ROWS);
  p.nchunks = D + nnz / GS_CHUNK;            // sum_d ceil(len_d / C) <= D + floor(nnz / C)
  const size_t GW = (size_t)p.LT * p.LT + p.LT;
  Carver c(ws);
  float* mT = c.take<float>((size_t)B * p.LT);
  float* wiv = c.take<float>((size_t)D * p.LT);
  double* spart = c.take<double>((size_t)p.nbS * GW);
  double* gpart = c.take<double>((size_t)p.nbG * GW);
  double* ssum = c.take<double>(GW);
  double* gsum = c.take<double>(GW);
  double* S2 = c.take<double>(GS_MAXL);
  int32_t* cstart = c.take<int32_t>((size_t)D + 1);
  int32_t* chunk_gene = c.take<int32_t>((size_t)p.nchunks);
  double* partv = c.take<double>((size_t)p.nchunks * p.LT);
  double* parts = c.take<double>((size_t)p.nchunks * 4);
  double* llg = c.take<double>((size_t)D);
  p.bytes = c.used();
  if (a) {
    a->mT = mT; a->wiv = wiv; a->spart = spart; a->gpart = gpart; a->ssum = ssum; a->gsum = gsum; a->S2 = S2;
    a->cstart = cstart; a->chunk_gene = chunk_gene; a->partv = partv; a->parts = parts; a->llg = llg;
    a->LT = p.LT; a->nbS = p.nbS; a->nbG = p.nbG; a->nchunks = p.nchunks;
  }
  return p;
}

static int gs_check_shape(const char* who, int64_t N, int64_t B, int64_t D, int Lt, int64_t nnz) {
  GPZ_REQUIRE(N >= 1 && B >= 1 && D >= 1 && nnz >= 0, "%s: bad extents (N = %lld, B = %lld, D = %lld, nnz = %lld)", who,
              (long long)N, (long long)B, (long long)D, (long long)nnz);
  GPZ_REQUIRE(B <= N, "%s: a batch of %lld distinct spots out of %lld", who, (long long)B, (long long)N);
  GPZ_REQUIRE(Lt >= 1 && Lt <= GS_MAXL, "%s: %d factors unsupported (1..%d)", who, Lt, GS_MAXL);
  GPZ_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && nnz < (1ll << 31) && D + nnz / GS_CHUNK < (1ll << 31),
              "%s: spots, genes and non-zeros are indexed with 32 bits", who);
  return 0;
}

template <int LT>
static int gs_passes(const GsArgs& a, hipStream_t s) {
  if (a.grads) {
    hipLaunchKernelGGL((gs_spot_kernel<LT>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, s, a);
    GPZ_LAUNCH_OK();
  }
  hipLaunchKernelGGL((gs_gene_kernel<LT>), dim3((unsigned)((a.nchunks + 3) / 4)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}

}  // namespace gsp
}  // namespace gpz

using namespace gpz;
using namespace gpz::gsp;

extern "C" int gpz_gaussian_fa_sparse_plan(int64_t N, int64_t B, int64_t D, int32_t Lt, int64_t nnz, int32_t* gene_chunk,
                                           int64_t* n_gene_chunks, int32_t* factors_padded, int64_t* workspace_bytes) {
  if (int rc = gs_check_shape("gpz_gaussian_fa_sparse", N, B, D, Lt, nnz)) return rc;
  const GsPlan p = gs_plan(B, D, Lt, nnz, nullptr, nullptr);
  if (gene_chunk) *gene_chunk = GS_CHUNK;
  if (n_gene_chunks) *n_gene_chunks = p.nchunks;
  if (factors_padded) *factors_padded = p.LT;
  if (workspace_bytes) *workspace_bytes = (int64_t)p.bytes;
  return 0;
}

extern "C" int gpz_gaussian_fa_sparse(const float* mean, const float* scale, const float* W, const float* b, const float* noise_sd,
                                      const double* offset, const int64_t* col_ptr, const int32_t* col_gene, const float* col_val,
                                      const int64_t* row_ptr, const int32_t* row_spot, const int32_t* row_perm,
                                      const int32_t* idx, const int32_t* pos, int64_t N, int64_t B, int64_t D, int64_t nnz,
                                      int32_t Lt, double* loglik, double* sse_per_gene, double* ss_per_gene, float* dmean,
                                      float* dscale, float* dW, float* db, float* dnoise_sd, void* partials,
                                      size_t partials_bytes, void* stream) {
  GPZ_REQUIRE(mean && scale && W && b && noise_sd && offset && col_ptr && row_ptr && loglik && partials,
              "gpz_gaussian_fa_sparse: null pointer");
  const int ngrad = (dmean != nullptr) + (dscale != nullptr) + (dW != nullptr) + (db != nullptr) + (dnoise_sd != nullptr);
  GPZ_REQUIRE(ngrad == 0 || ngrad == 5, "gpz_gaussian_fa_sparse: the five gradient pointers must be all null or all set");
  if (int rc = gs_check_shape("gpz_gaussian_fa_sparse", N, B, D, Lt, nnz)) return rc;
  GPZ_REQUIRE(nnz == 0 || (col_gene && col_val && row_spot && row_perm), "gpz_gaussian_fa_sparse: null pointer (non-zeros)");
  GPZ_REQUIRE((idx == nullptr) == (pos == nullptr), "gpz_gaussian_fa_sparse: idx and pos come together (both null: all spots)");
  GPZ_REQUIRE(idx || B == N, "gpz_gaussian_fa_sparse: B = %lld of N = %lld spots needs idx and pos", (long long)B, (long long)N);
  // the scratch memory is carved into aligned pieces that are read 16 bytes at a time; the inputs are read element by element
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 15) == 0, "gpz_gaussian_fa_sparse: partials must be 16-byte aligned");
  GPZ_REQUIRE((reinterpret_cast<uintptr_t>(offset) & 7) == 0, "gpz_gaussian_fa_sparse: offset must be 8-byte aligned");
  GsArgs a;
  const GsPlan p = gs_plan(B, D, Lt, nnz, &a, partials);
  GPZ_REQUIRE(partials_bytes >= p.bytes, "gpz_gaussian_fa_sparse: partials too small (%zu bytes, %zu needed)", partials_bytes, p.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  a.mean = mean; a.scale = scale; a.W = W; a.b = b; a.sd = noise_sd; a.offset = offset;
  a.col_ptr = col_ptr; a.col_gene = col_gene; a.col_val = col_val;
  a.row_ptr = row_ptr; a.row_spot = row_spot; a.row_perm = row_perm; a.idx = idx; a.pos = pos;
  a.loglik = loglik; a.sse = sse_per_gene; a.ss = ss_per_gene;
  a.dmean = dmean; a.dscale = dscale; a.dW = dW; a.db = db; a.dsd = dnoise_sd;
  a.N = N; a.B = B; a.D = D; a.nnz = nnz; a.Lt = Lt; a.grads = ngrad == 5;
  const int GW = a.LT * a.LT + a.LT;
  hipLaunchKernelGGL(gs_mt_kernel, dim3((unsigned)((B + 63) / 64)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(gs_s2_kernel, dim3(GS_MAXL), dim3(1024), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(gs_gram_kernel, dim3((unsigned)a.nbS), dim3(256), 0, s, a, 0);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(gs_reduce_kernel, dim3((unsigned)((GW + 255) / 256)), dim3(256), 0, s, a.spart, a.nbS, GW, a.ssum);
  GPZ_LAUNCH_OK();
  if (a.grads) {
    hipLaunchKernelGGL(gs_wiv_kernel, dim3((unsigned)((D * a.LT + 255) / 256)), dim3(256), 0, s, a);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL(gs_gram_kernel, dim3((unsigned)a.nbG), dim3(256), 0, s, a, 1);
    GPZ_LAUNCH_OK();
    hipLaunchKernelGGL(gs_reduce_kernel, dim3((unsigned)((GW + 255) / 256)), dim3(256), 0, s, a.gpart, a.nbG, GW, a.gsum);
    GPZ_LAUNCH_OK();
  }
  hipLaunchKernelGGL(chunks_kernel, dim3(1), dim3(1024), 0, s, a.row_ptr, a.D, a.nchunks, GS_CHUNK, true, a.cstart, a.chunk_gene);
  GPZ_LAUNCH_OK();
  int rc;
  switch (a.LT) {
    case 4: rc = gs_passes<4>(a, s); break;
    case 8: rc = gs_passes<8>(a, s); break;
    case 12: rc = gs_passes<12>(a, s); break;
    case 16: rc = gs_passes<16>(a, s); break;
    case 20: rc = gs_passes<20>(a, s); break;
    case 24: rc = gs_passes<24>(a, s); break;
    case 32: rc = gs_passes<32>(a, s); break;
    case 40: rc = gs_passes<40>(a, s); break;
    case 48: rc = gs_passes<48>(a, s); break;
    default: rc = gs_passes<64>(a, s); break;
  }
  if (rc) return rc;
  hipLaunchKernelGGL(gs_finish_kernel, dim3((unsigned)((D + GS_GENES - 1) / GS_GENES)), dim3(256), 0, s, a);
  GPZ_LAUNCH_OK();
  hipLaunchKernelGGL(gs_total_kernel, dim3(1), dim3(1024), 0, s, a);
  GPZ_LAUNCH_OK();
  return 0;
}
