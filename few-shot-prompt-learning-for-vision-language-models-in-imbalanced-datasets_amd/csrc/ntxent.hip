// NT-Xent (SimCLR) loss on two views, forward and gradient (clipk_ntxent_loss, include/clipk.h):
// LogitsNTXentLoss (PromptSRC/trainers/coop.py:72-123) and ImageNTXentLoss (independentVL.py:73-112).
//
// Rows x_0..x_{N-1} = the rows of a, then of b (N = 2n); p(i) = (i + n) mod N.
//   r_i = 1 / max(|x_i|, 1e-12)   z_i = r_i x_i   s_ij = z_i . z_j / T
//   L_i = log sum_{j != i} exp(s_ij) - s_{i,p(i)}             loss = (1/N) sum_i L_i
//   P_ij = exp(s_ij - lse_i) (j != i)   W_ij = (P_ij + P_ji - 2 [j == p(i)]) / N   c_i = sum_j W_ij s_ij
//   dL/dx_i = sum_j (r_i r_j W_ij / T) x_j - c_i r_i^2 x_i
//
// Three launches, data handed on at kernel boundaries only:
//  1. gram_kernel    raw Gram matrix g_ij = x_i . x_j (fp32 FMA chains), 16 MT x 16 MT output tiles,
//                    D cut into slices (grid z) so that small N still fills the device; slice
//                    partials go to the workspace. |x_i|^2 is the diagonal, so no norm pass exists.
//  2. rows_kernel    one wave per row: the slices summed in slice order, s_ij (stored, bitwise
//                    symmetric), the row's logsumexp over j != i as the pair (max_i, log sum exp(s -
//                    max_i)) -- kept apart, as log_softmax does: the sum max + log rounds at the
//                    ulp of s ~ 1/T and put 4x that error into every P -- r_i and L_i.
//  3. grad_kernel    dX = A X as a second tiled product over j, with A_ij = grad_scale r_i r_j W_ij / T
//                    formed tile by tile from s, lse and r as it is staged (two exp per element),
//                    c_i accumulated on the way in a fixed order; its block (0, 0) also sums the
//                    L_i into the loss. Forward only: loss_kernel does that sum instead.
// No atomics, every sum in a fixed order: results are bitwise reproducible.
//
// Global loads are unconditional on clamped (always in-bounds) indices and a select drops what
// lies outside: a load under a per-lane condition compiles to a branch with its own wait, and
// the loaders' 16 loads per stage then ran one round trip after the other. The two tiled kernels
// also fetch the next stage into registers while they compute the current one from LDS.
#include "common.h"

using namespace clipk;

namespace {

constexpr int KC = 32;      // reduction-dimension elements per LDS stage
constexpr int RS = KC + 4;  // LDS row stride in floats: rows stay 16-B aligned and shift by 4 banks
constexpr int kMaxN = 1024; // N = 2n rows at most (n <= 512)

struct Plan {
  int mt;      // micro-tile edge per thread: 16 mt x 16 mt output tiles
  int splits;  // D slices of the Gram product
  int kchunk;  // D elements per slice (multiple of KC)
};

// Small N: 32 x 32 tiles and as many D slices as it takes to reach ~256 blocks (one per CU).
Plan make_plan(int N, int D) {
  Plan p;
  p.mt = N >= 256 ? 4 : 2;
  const int T = 16 * p.mt;
  const int tiles = ((N + T - 1) / T) * ((N + T - 1) / T);
  const int chunks = (D + KC - 1) / KC;
  int want = 256 / tiles;
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  int splits = want < chunks ? want : chunks;
  p.kchunk = ((chunks + splits - 1) / splits) * KC;
  p.splits = (D + p.kchunk - 1) / p.kchunk;
  return p;
}

__device__ __forceinline__ const float* row_ptr(const float* a, const float* b, int n, int D, int i) {
  return i < n ? a + (size_t)i * D : b + (size_t)(i - n) * D;
}

// part[z][i][j] = sum_{k in slice z} x_i[k] x_j[k]. Thread (tx, ty) owns rows ty + 16 m and columns
// tx + 16 c of the tile (row stride RS in LDS: the 16 lanes of a b128 read hit distinct banks).
// g_ij and g_ji come from the same fmaf chain with commuted factors: bitwise equal.
template <int MT>
__global__ __launch_bounds__(256) void gram_kernel(int n, int D, int kchunk, const float* __restrict__ a,
                                                   const float* __restrict__ b, float* __restrict__ part) {
  constexpr int T = 16 * MT;
  constexpr int P = T / 8;  // loader passes of 8 rows
  __shared__ CLIPK_LDS_ALIGN float As[T * RS];
  __shared__ CLIPK_LDS_ALIGN float Bs[T * RS];
  const int N = 2 * n;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int lk = t & 31, lr = t >> 5;  // loader: k within the stage, row within a pass
  const int I0 = blockIdx.y * T, J0 = blockIdx.x * T;
  const int k0 = blockIdx.z * kchunk;
  const int k1 = min(D, k0 + kchunk);
  const float* pa[P];
  const float* pb[P];
  bool va[P], vb[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = I0 + p * 8 + lr, j = J0 + p * 8 + lr;
    va[p] = i < N;
    vb[p] = j < N;
    pa[p] = row_ptr(a, b, n, D, min(i, N - 1));
    pb[p] = row_ptr(a, b, n, D, min(j, N - 1));
  }
  float ra[P], rb[P];
  auto fetch = [&](int ks) {
    const int k = min(ks + lk, k1 - 1);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      ra[p] = pa[p][k];
      rb[p] = pb[p][k];
    }
  };
  float acc[MT][MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int c = 0; c < MT; ++c) acc[m][c] = 0.f;
  fetch(k0);
  for (int ks = k0; ks < k1; ks += KC) {
    const bool kv = ks + lk < k1;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      As[(p * 8 + lr) * RS + lk] = (va[p] && kv) ? ra[p] : 0.f;
      Bs[(p * 8 + lr) * RS + lk] = (vb[p] && kv) ? rb[p] : 0.f;
    }
    __syncthreads();
    if (ks + KC < k1) fetch(ks + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      f32x4 av[MT], bv[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) av[m] = *reinterpret_cast<const f32x4*>(&As[(ty + 16 * m) * RS + kk]);
#pragma unroll
      for (int c = 0; c < MT; ++c) bv[c] = *reinterpret_cast<const f32x4*>(&Bs[(tx + 16 * c) * RS + kk]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int c = 0; c < MT; ++c) acc[m][c] = fmaf(av[m][e], bv[c][e], acc[m][c]);
    }
    __syncthreads();
  }
  float* out = part + (size_t)blockIdx.z * N * N;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int i = I0 + ty + 16 * m;
#pragma unroll
    for (int c = 0; c < MT; ++c) {
      const int j = J0 + tx + 16 * c;
      if (i < N && j < N) out[(size_t)i * N + j] = acc[m][c];
    }
  }
}

// Wave per row i (N <= 64 Q columns, Q per lane): g = the slice partials summed in slice order;
// s_ij = g_ij (r_i r_j) / T (the product r_i r_j commutes, so S stays bitwise symmetric); lse_i
// over j != i as (rmax_i, rlog_i); L_i = (rmax_i - s_{i,p(i)}) + rlog_i. The slice sums fetch 32 partials per lane at a time (KB slices of Q columns)
// and add them in slice order; slices past the last are fetched clamped and added as zeros.
template <int Q>
__global__ __launch_bounds__(256) void rows_kernel(int n, int splits, float inv_t, const float* __restrict__ part,
                                                   float* __restrict__ S, float* __restrict__ rmax,
                                                   float* __restrict__ rlog, float* __restrict__ rinv,
                                                   float* __restrict__ rowloss) {
  constexpr int KB = 32 / Q;
  constexpr int M0 = (64 * Q + 255) / 256;  // diagonal entries per thread
  __shared__ float rs[64 * Q];
  const int N = 2 * n;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const size_t NN = (size_t)N * N;
  {  // r_j of every row from the diagonal, by the whole block
    float g[M0];
    size_t off[M0];
#pragma unroll
    for (int m = 0; m < M0; ++m) {
      g[m] = 0.f;
      off[m] = (size_t)min((int)threadIdx.x + 256 * m, N - 1) * (N + 1);
    }
    for (int k0 = 0; k0 < splits; k0 += 8) {
      float v[8][M0];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int m = 0; m < M0; ++m) v[u][m] = part[(size_t)min(k0 + u, splits - 1) * NN + off[m]];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int m = 0; m < M0; ++m) g[m] += (k0 + u < splits) ? v[u][m] : 0.f;
    }
#pragma unroll
    for (int m = 0; m < M0; ++m) {
      const int j = threadIdx.x + 256 * m;
      if (j < N) rs[j] = 1.0f / fmaxf(sqrtf(g[m]), 1e-12f);  // F.normalize's clamp
    }
  }
  __syncthreads();
  if (i >= N) return;
  const float ri = rs[i];
  const int pi = i < n ? i + n : i - n;
  const float* row = part + (size_t)i * N;
  int jc[Q];
  float acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    jc[q] = min(lane + 64 * q, N - 1);
    acc[q] = 0.f;
  }
  for (int k0 = 0; k0 < splits; k0 += KB) {
    float v[KB][Q];
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int q = 0; q < Q; ++q) v[u][q] = row[(size_t)min(k0 + u, splits - 1) * NN + jc[q]];
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] += (k0 + u < splits) ? v[u][q] : 0.f;
  }
  float s[Q];
  float mx = -INFINITY, spos = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int j = lane + 64 * q;
    const float v = acc[q] * (ri * rs[jc[q]]) * inv_t;
    if (j < N) S[(size_t)i * N + j] = v;
    spos += (j == pi) ? v : 0.f;  // (pi < N: a clamped duplicate column never matches twice)
    s[q] = (j < N && j != i) ? v : -INFINITY;
    mx = fmaxf(mx, s[q]);
  }
  mx = wave_max(mx);  // finite: N >= 2 leaves every row its positive
  float se = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) se += expf(s[q] - mx);  // excluded entries: exp(-inf) = 0
  se = wave_sum(se);
  spos = wave_sum(spos);  // one lane holds it, the others add zeros
  const float lg = logf(se);
  if (lane == 0) {
    rmax[i] = mx;
    rlog[i] = lg;
    rinv[i] = ri;
    rowloss[i] = (mx - spos) + lg;
  }
}

// loss = (1/N) sum_i L_i by one wave: lane l sums rows l, l + 64, ... in order, then the butterfly.
__device__ __forceinline__ void loss_reduce(int N, const float* __restrict__ rowloss, float* __restrict__ loss) {
  const int lane = threadIdx.x;
  float v = 0.f;
  for (int i = lane; i < N; i += 64) v += rowloss[i];
  v = wave_sum(v);
  if (lane == 0) loss[0] = v * (1.0f / (float)N);
}

__global__ __launch_bounds__(64) void loss_kernel(int N, const float* __restrict__ rowloss, float* __restrict__ loss) {
  loss_reduce(N, rowloss, loss);
}

// dX tile [16 MT rows of X, 16 MT columns of D] = sum_j A_ij x_j - gs c_i r_i^2 x_i. Per stage of KC
// columns j the A tile is formed from S, lse = (rmax, rlog) and r (lane = j within the stage:
// coalesced S reads; P_ij = exp((s_ij - rmax_i) - rlog_i), P_ji likewise from row j's pair by symmetry)
// and the matching rows of X staged as Xs[j][d]. Each loader thread keeps its rows' share of c_i;
// the 32 lanes of a row are summed by a butterfly at the end (fixed order).
template <int MT>
__global__ __launch_bounds__(256) void grad_kernel(int n, int D, float inv_t, float gs, const float* __restrict__ a,
                                                   const float* __restrict__ b, const float* __restrict__ S,
                                                   const float* __restrict__ rmax, const float* __restrict__ rlog,
                                                   const float* __restrict__ rinv, const float* __restrict__ rowloss,
                                                   float* __restrict__ loss,
                                                   float* __restrict__ da, float* __restrict__ db) {
  constexpr int T = 16 * MT;
  constexpr int P = T / 8;     // A-tile loader passes (8 rows each)
  constexpr int XR = 256 / T;  // X-tile rows per loader pass
  constexpr int XP = KC / XR;  // X-tile loader passes
  __shared__ CLIPK_LDS_ALIGN float As[T * RS];
  __shared__ float Xs[KC * T];
  __shared__ float cs[T];
  const int N = 2 * n;
  const float inv_n = 1.0f / (float)N;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int lk = t & 31, lr = t >> 5;
  const int xd = t % T, xr = t / T;
  const int I0 = blockIdx.y * T, d0 = blockIdx.x * T;
  const bool dv = d0 + xd < D;
  const int dc = min(d0 + xd, D - 1);
  int soff[P];  // row offsets into S (N * N <= 2^20)
  float mi[P], gi[P], rri[P], cacc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int ic = min(I0 + p * 8 + lr, N - 1);
    soff[p] = ic * N;
    mi[p] = rmax[ic];
    gi[p] = rlog[ic];
    rri[p] = rinv[ic];
    cacc[p] = 0.f;
  }
  float sv[P], xv[XP], mj, gj, rj;
  auto fetch = [&](int j0) {
    const int jc = min(j0 + lk, N - 1);
    mj = rmax[jc];
    gj = rlog[jc];
    rj = rinv[jc];
#pragma unroll
    for (int p = 0; p < P; ++p) sv[p] = S[soff[p] + jc];
#pragma unroll
    for (int p = 0; p < XP; ++p) xv[p] = row_ptr(a, b, n, D, min(j0 + p * XR + xr, N - 1))[dc];
  };
  float acc[MT][MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int c = 0; c < MT; ++c) acc[m][c] = 0.f;
  const float ascale = gs * inv_t;
  fetch(0);
  for (int j0 = 0; j0 < N; j0 += KC) {
    const int j = j0 + lk;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int il = p * 8 + lr;
      const int i = I0 + il;
      const int pi = i < n ? i + n : i - n;
      const bool ok = i < N && j < N && j != i;
      const float s = sv[p];
      float w = (expf((s - mi[p]) - gi[p]) + expf((s - mj) - gj) - (j == pi ? 2.0f : 0.0f)) * inv_n;
      w = ok ? w : 0.f;
      cacc[p] = fmaf(w, s, cacc[p]);
      As[il * RS + lk] = ok ? ascale * (rri[p] * rj) * w : 0.f;
    }
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const int jl = p * XR + xr;
      Xs[jl * T + xd] = (dv && j0 + jl < N) ? xv[p] : 0.f;
    }
    __syncthreads();
    if (j0 + KC < N) fetch(j0 + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      f32x4 av[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) av[m] = *reinterpret_cast<const f32x4*>(&As[(ty + 16 * m) * RS + kk]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float xe[MT];
#pragma unroll
        for (int c = 0; c < MT; ++c) xe[c] = Xs[(kk + e) * T + tx + 16 * c];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int c = 0; c < MT; ++c) acc[m][c] = fmaf(av[m][e], xe[c], acc[m][c]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    float v = cacc[p];
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lk == 0) cs[p * 8 + lr] = v;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int il = ty + 16 * m;
    const int i = I0 + il;
    if (i >= N) continue;
    const float ri = rinv[i];
    const float coef = gs * cs[il] * ri * ri;
    const float* x = row_ptr(a, b, n, D, i);
    float* out = i < n ? da + (size_t)i * D : db + (size_t)(i - n) * D;
#pragma unroll
    for (int c = 0; c < MT; ++c) {
      const int d = d0 + tx + 16 * c;
      if (d < D) out[d] = acc[m][c] - coef * x[d];
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && t < 64) loss_reduce(N, rowloss, loss);
}

size_t ws_floats(int N, const Plan& p) { return (size_t)(p.splits + 1) * N * N + 4 * (size_t)N; }

}  // namespace

extern "C" size_t clipk_ntxent_ws_bytes(int n, int D) {
  if (n < 1 || n > kMaxN / 2 || D < 1) return 0;
  const Plan p = make_plan(2 * n, D);
  return (ws_floats(2 * n, p) * sizeof(float) + 255) / 256 * 256;
}

extern "C" int clipk_ntxent_loss(int n, int D, const float* a, const float* b, float temperature, float grad_scale,
                                 float* loss, float* da, float* db, void* ws, void* stream) {
  if (!a || !b || !loss || !ws || !(temperature > 0.f)) return CLIPK_EINVAL;
  if ((da == nullptr) != (db == nullptr) || (uintptr_t)ws % sizeof(float)) return CLIPK_EINVAL;
  if (n < 1 || n > kMaxN / 2 || D < 1) return CLIPK_ESHAPE;
  const int N = 2 * n;
  const Plan p = make_plan(N, D);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  float* S = part + (size_t)p.splits * N * N;
  float* rmax = S + (size_t)N * N;
  float* rlog = rmax + N;
  float* rinv = rlog + N;
  float* rowloss = rinv + N;
  const float inv_t = 1.0f / temperature;
  const int T = 16 * p.mt;
  const int tiles = (N + T - 1) / T;
  if (p.mt == 4)
    hipLaunchKernelGGL(gram_kernel<4>, dim3(tiles, tiles, p.splits), dim3(256), 0, st, n, D, p.kchunk, a, b, part);
  else
    hipLaunchKernelGGL(gram_kernel<2>, dim3(tiles, tiles, p.splits), dim3(256), 0, st, n, D, p.kchunk, a, b, part);
  CLIPK_CHECK_LAUNCH();
  const dim3 rgrid((N + 3) / 4);
#define CLIPK_ROWS(Q) \
  hipLaunchKernelGGL(rows_kernel<Q>, rgrid, dim3(256), 0, st, n, p.splits, inv_t, part, S, rmax, rlog, rinv, rowloss)
  if (N <= 64) CLIPK_ROWS(1);
  else if (N <= 128) CLIPK_ROWS(2);
  else if (N <= 256) CLIPK_ROWS(4);
  else if (N <= 512) CLIPK_ROWS(8);
  else CLIPK_ROWS(16);
#undef CLIPK_ROWS
  CLIPK_CHECK_LAUNCH();
  if (!da) {
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(64), 0, st, N, rowloss, loss);
    CLIPK_CHECK_LAUNCH();
    return CLIPK_OK;
  }
  // the gradient product has no reduction slices to spread: 64 x 64 tiles only where they fill the
  // device on their own ((256, 512): 64 of them ran 44 us, a quarter of the CUs busy)
  const int gmt = (size_t)((N + 63) / 64) * ((D + 63) / 64) >= 256 ? 4 : 2;
  const int GT = 16 * gmt;
  const dim3 grid((D + GT - 1) / GT, (N + GT - 1) / GT);
  if (gmt == 4)
    hipLaunchKernelGGL(grad_kernel<4>, grid, dim3(256), 0, st, n, D, inv_t, grad_scale, a, b, S, rmax, rlog, rinv,
                       rowloss, loss, da, db);
  else
    hipLaunchKernelGGL(grad_kernel<2>, grid, dim3(256), 0, st, n, D, inv_t, grad_scale, a, b, S, rmax, rlog, rinv,
                       rowloss, loss, da, db);
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}
