// LoRA on attn.in_proj_weight (this package's LoRA trainer; include/clipk.h clipk_lora_*).
//
//   W'_p = W0_p + s B_p A_p   for the enabled projections p of q | k | v   (A_p [r, W], B_p [W, r])
//
// The encoders run on the merged W' (LoRA is linear: the existing forward and input-grad GEMMs on
// W' / W'^T are LoRA's own), so two things are new:
//
//  clipk_lora_merge   one launch per encoder, grid z = layer: W' [3W, W] in the act dtype and
//                     W'^T [W, 3W] in the grad dtype from the same registers, the transpose through
//                     a 64 x 64 LDS tile. acc = 0; acc = fma(B[n, j], A[j, k], acc) for j ascending;
//                     out = fma(s, acc, W0[n, k]); one rounding to each output dtype.
//  clipk_lora_wgrad   the adapters' own gradient for one layer, from the saved layer input X, its
//                     LayerNorm statistics and dqkv = dY:
//                        xn = LN1(X)   P_p = xn A_p^T   dU_p = s dY_p B_p
//                        dB_p = s dY_p^T P_p            dA_p = dU_p^T xn
//                     Three launches: (1) rows_kernel, 32 rows per block: P and dU [rows, 3r] fp32
//                     into the workspace; (2) part_kernel, one wave per (64 columns, row chunk):
//                     the chunk's partial dA / dB, rows in order, xn recomputed from X (so X and dY
//                     are streamed twice and xn is never stored); (3) final_kernel: the chunks summed
//                     in order, s applied to dB, zeros for the disabled projections.
// Products on the fp32 VALU, not on MFMA ("LoRA kernels"): one side of every product is
// 3 r <= 48 wide (6 at the default rank), so an MFMA tile would be mostly padding, the f32-input
// MFMA runs at the VALU's rate anyway, and the 16-bit one would round xn / dU / P. No atomics, every
// sum in an order fixed by the shapes: bitwise reproducible. Global loads are unconditional on
// clamped (always in-bounds) indices, with a select for rows past the end.
#include "common.h"

using namespace clipk;

namespace {

constexpr int kMaxLayers = 32;
constexpr int kMaxRank = 16;

// ---------------------------------------------------------------- merge
struct MergePtrs {
  const float* w0[kMaxLayers];
  void* out[kMaxLayers];
  void* outT[kMaxLayers];
};

constexpr int MT = 64;  // merge tile edge

// Block (kt, nt, layer): rows n = 64 nt .. + 63 of [3W] (one projection: W % 64 == 0), columns
// k = 64 kt .. + 63. Thread (tx, ty) owns columns 4 tx .. + 3 of rows ty + 16 m.
template <typename TA, typename TG>
__global__ __launch_bounds__(256) void merge_kernel(int W, int r, unsigned proj_mask, unsigned layer_mask, float s,
                                                    MergePtrs ptrs, const float* __restrict__ A,
                                                    const float* __restrict__ B) {
  __shared__ float ts[MT * (MT + 1)];  // [k][n]
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int l = blockIdx.z;
  const int n0 = blockIdx.y * MT, k0 = blockIdx.x * MT;
  const int p = n0 / W;
  const bool on = ((layer_mask >> l) & 1u) && ((proj_mask >> p) & 1u);
  const float* __restrict__ w0 = ptrs.w0[l];
  const float* __restrict__ Ap = A + ((size_t)l * 3 + p) * r * W;
  const float* __restrict__ Bp = B + ((size_t)l * 3 + p) * W * r;
  TA* __restrict__ out = (TA*)ptrs.out[l];
  TG* __restrict__ outT = (TG*)ptrs.outT[l];
  const int k = k0 + 4 * tx;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int n = n0 + ty + 16 * m;
    f32x4 v = *reinterpret_cast<const f32x4*>(w0 + (size_t)n * W + k);
    if (on) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* brow = Bp + (size_t)(n - p * W) * r;
      for (int j = 0; j < r; ++j) {
        const float b = brow[j];
        const f32x4 a = *reinterpret_cast<const f32x4*>(Ap + (size_t)j * W + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(b, a[i], acc[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaf(s, acc[i], v[i]);
    }
    store4<TA>(out + (size_t)n * W + k, v[0], v[1], v[2], v[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) ts[(4 * tx + i) * (MT + 1) + ty + 16 * m] = v[i];
  }
  if (!outT) return;  // (uniform: a forward-only table)
  __syncthreads();
  // W'^T [W, 3W]: thread (tx, ty) writes columns n0 + 4 tx .. + 3 of rows k0 + ty + 16 m
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int kk = ty + 16 * m;
    const float* row = &ts[kk * (MT + 1) + 4 * tx];
    store4<TG>(outT + (size_t)(k0 + kk) * 3 * W + n0 + 4 * tx, row[0], row[1], row[2], row[3]);
  }
}

template <typename TA>
int merge_launch_g(int gd, dim3 grid, hipStream_t st, int W, int r, unsigned pm, unsigned lm, float s,
                   const MergePtrs& ptrs, const float* A, const float* B) {
#define CLIPK_LORA_MERGE(TG) hipLaunchKernelGGL((merge_kernel<TA, TG>), grid, dim3(256), 0, st, W, r, pm, lm, s, ptrs, A, B)
  if (gd == CLIPK_F32) CLIPK_LORA_MERGE(float);
  else if (gd == CLIPK_F16) CLIPK_LORA_MERGE(f16);
  else if (gd == CLIPK_BF16) CLIPK_LORA_MERGE(bf16);
  else return CLIPK_EDTYPE;
#undef CLIPK_LORA_MERGE
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

// ---------------------------------------------------------------- wgrad
constexpr int RT = 32;      // rows per block of the rows pass
constexpr int KC = 32;      // reduction elements per LDS stage
constexpr int XS = KC + 1;  // row stride of the staged activations (floats): lanes walk rows
constexpr int kChunk = 32;  // rows per chunk of the partial sums (more when rows > 32768)
constexpr int kMaxChunks = 1024;

int chunk_rows(int rows) {
  const int c = (rows + kMaxChunks - 1) / kMaxChunks;
  return c > kChunk ? c : kChunk;
}

struct Ws {
  float *P, *dU, *pA, *pB;
  int ch, nch;
  size_t floats;
};

// base may be null (clipk_lora_wgrad_ws_bytes): only floats is meaningful then.
Ws carve(float* base, int rows, int W, int r) {
  Ws w;
  size_t o = 0;
  auto take = [&](size_t n) {
    float* f = base ? base + o : nullptr;
    o += (n + 3) / 4 * 4;
    return f;
  };
  w.ch = chunk_rows(rows);
  w.nch = (rows + w.ch - 1) / w.ch;
  w.P = take((size_t)rows * 3 * r);
  w.dU = take((size_t)rows * 3 * r);
  w.pA = take((size_t)w.nch * 3 * r * W);
  w.pB = take((size_t)w.nch * 3 * W * r);
  w.floats = o;
  return w;
}

// Rows pass. Block (b, ph): rows 32 b .. + 31; ph 0 forms P, ph 1 + p forms dU of projection p
// (a disabled one returns at once), so the grid is four times the row tiles and each block's
// chain of stages a quarter of the work. Loader: thread t stages elements 4 (t & 7) .. + 3 of row
// t >> 3 of a 32 x 32 stage, the next stage's global loads issued before this stage's products
// (probe.hip's pipeline); thread (row = t & 31, g = t >> 5) owns the outputs g + 8 i of its row
// (the operand rows are uniform over each half wave: LDS broadcasts).
//   P[row][c]  = sum_k xn[row][k] A[c][k]                c = p r + j over [3r][W] (A's own layout)
//   dU[row][c] = s sum_n dY[row][p W + n] B[p][n][j]
template <typename TX, typename TG, int RP>
__global__ __launch_bounds__(256) void rows_kernel(int rows, int W, int r, unsigned proj_mask, float s,
                                                   const TX* __restrict__ X, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const TG* __restrict__ dY,
                                                   const float* __restrict__ A, const float* __restrict__ B,
                                                   float* __restrict__ P, float* __restrict__ dU) {
  constexpr int NP = (3 * RP + 7) / 8;  // outputs of P per thread
  constexpr int NU = (RP + 7) / 8;      // outputs of dU per thread
  __shared__ float xs[RT * XS];
  __shared__ CLIPK_LDS_ALIGN float as[3 * kMaxRank * KC];
  const int t = threadIdx.x;
  const int row = t & 31, g = t >> 5;
  const int lr = t >> 3, lk = (t & 7) * 4;
  const int R0 = blockIdx.x * RT;
  const int grow = min(R0 + lr, rows - 1);  // the loader's row, clamped
  const int r3 = 3 * r;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (blockIdx.y == 0) {
    const float mu = mean[grow], rs = rstd[grow];
    const TX* xrow = X + (size_t)grow * W;
    const int na = r3 * (KC / 4);  // 16-byte pieces of the A stage: piece i = row i / 8, quad i % 8
    float v[4];
    f32x4 gm, bt, a0 = zero, a1 = zero;
    auto fetch = [&](int k0) {
      load4<TX>(xrow + k0 + lk, v);
      gm = *reinterpret_cast<const f32x4*>(gamma + k0 + lk);
      bt = *reinterpret_cast<const f32x4*>(beta + k0 + lk);
      if (t < na) a0 = *reinterpret_cast<const f32x4*>(A + (size_t)(t >> 3) * W + k0 + (t & 7) * 4);
      if (t + 256 < na) a1 = *reinterpret_cast<const f32x4*>(A + (size_t)((t + 256) >> 3) * W + k0 + (t & 7) * 4);
    };
    fetch(0);
    float acc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < W; k0 += KC) {
#pragma unroll
      for (int i = 0; i < 4; ++i) xs[lr * XS + lk + i] = (v[i] - mu) * rs * gm[i] + bt[i];
      if (t < na) *reinterpret_cast<f32x4*>(&as[4 * t]) = a0;
      if (t + 256 < na) *reinterpret_cast<f32x4*>(&as[4 * (t + 256)]) = a1;
      __syncthreads();
      if (k0 + KC < W) fetch(k0 + KC);
#pragma unroll 8
      for (int kk = 0; kk < KC; ++kk) {
        const float x = xs[row * XS + kk];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int c = g + 8 * i;
          if (c < r3) acc[i] = fmaf(x, as[c * KC + kk], acc[i]);
        }
      }
      __syncthreads();
    }
    if (R0 + row < rows) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int c = g + 8 * i;
        if (c < r3) P[(size_t)(R0 + row) * r3 + c] = acc[i];
      }
    }
    return;
  }
  const int p = blockIdx.y - 1;
  if (!((proj_mask >> p) & 1u)) return;
  const TG* yrow = dY + (size_t)grow * 3 * W + (size_t)p * W;
  const float* Bp = B + (size_t)p * W * r;
  const int nb = KC * r / 4;  // 16-byte pieces of the B stage ([n][j], contiguous in B): <= 128
  float v[4];
  f32x4 b0 = zero;
  auto fetch = [&](int n0) {
    load4<TG>(yrow + n0 + lk, v);
    if (t < nb) b0 = *reinterpret_cast<const f32x4*>(Bp + (size_t)n0 * r + 4 * t);
  };
  fetch(0);
  float acc[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) acc[i] = 0.f;
  for (int n0 = 0; n0 < W; n0 += KC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) xs[lr * XS + lk + i] = v[i];
    if (t < nb) *reinterpret_cast<f32x4*>(&as[4 * t]) = b0;
    __syncthreads();
    if (n0 + KC < W) fetch(n0 + KC);
#pragma unroll 8
    for (int nn = 0; nn < KC; ++nn) {
      const float y = xs[row * XS + nn];
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int j = g + 8 * i;
        if (j < r) acc[i] = fmaf(y, as[nn * r + j], acc[i]);
      }
    }
    __syncthreads();
  }
  if (R0 + row < rows) {
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int j = g + 8 * i;
      if (j < r) dU[(size_t)(R0 + row) * r3 + p * r + j] = s * acc[i];
    }
  }
}

// Partial sums. One wave per block; block (ct, chunk): column tile ct < W / 64 is dA's columns
// k = 64 ct + lane (all three projections: they share xn), the 3 W / 64 tiles after them are dB's
// rows n3 = p W + n. Rows of the chunk in order, one fma chain per output; the loads of 8 rows are
// issued together.
//   pA[chunk][p][j][k] = sum_row dU[row][p r + j] xn[row][k]
//   pB[chunk][p][n][j] = sum_row dY[row][p W + n] P[row][p r + j]
template <typename TX, typename TG, int RP>
__global__ __launch_bounds__(64) void part_kernel(int rows, int W, int r, int ch, unsigned proj_mask,
                                                  const TX* __restrict__ X, const float* __restrict__ mean,
                                                  const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, const TG* __restrict__ dY,
                                                  const float* __restrict__ P, const float* __restrict__ dU,
                                                  float* __restrict__ pA, float* __restrict__ pB) {
  constexpr int UR = 8;
  const int lane = threadIdx.x;
  const int ct = blockIdx.x, c = blockIdx.y;
  const int ra = c * ch, rb = min(ra + ch, rows);
  const int r3 = 3 * r, nka = W / 64;
  if (ct < nka) {
    const int k = ct * 64 + lane;
    const float gm = gamma[k], bt = beta[k];
    float acc[3][RP];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int j = 0; j < RP; ++j) acc[p][j] = 0.f;
    for (int r0 = ra; r0 < rb; r0 += UR) {
      float xn[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int row = min(r0 + u, rb - 1);  // (clamped: the rows past the chunk are not added)
        xn[u] = (to_f32(X[(size_t)row * W + k]) - mean[row]) * rstd[row] * gm + bt;
      }
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        if (r0 + u >= rb) break;
        const float* uu = dU + (size_t)(r0 + u) * r3;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          if (!((proj_mask >> p) & 1u)) continue;
#pragma unroll
          for (int j = 0; j < RP; ++j)
            if (j < r) acc[p][j] = fmaf(uu[p * r + j], xn[u], acc[p][j]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      if (!((proj_mask >> p) & 1u)) continue;
#pragma unroll
      for (int j = 0; j < RP; ++j)
        if (j < r) pA[(((size_t)c * 3 + p) * r + j) * W + k] = acc[p][j];
    }
  } else {
    const int n3 = (ct - nka) * 64 + lane;
    const int p = n3 / W;  // wave-uniform: W % 64 == 0
    if (!((proj_mask >> p) & 1u)) return;
    float acc[RP];
#pragma unroll
    for (int j = 0; j < RP; ++j) acc[j] = 0.f;
    for (int r0 = ra; r0 < rb; r0 += UR) {
      float y[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) y[u] = to_f32(dY[(size_t)min(r0 + u, rb - 1) * 3 * W + n3]);
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        if (r0 + u >= rb) break;
        const float* pp = P + (size_t)(r0 + u) * r3 + p * r;
#pragma unroll
        for (int j = 0; j < RP; ++j)
          if (j < r) acc[j] = fmaf(y[u], pp[j], acc[j]);
      }
    }
    float* o = pB + ((size_t)c * 3 * W + n3) * r;
#pragma unroll
    for (int j = 0; j < RP; ++j)
      if (j < r) o[j] = acc[j];
  }
}

// dA[i] = sum_chunk pA[chunk][i], dB[i] = s sum_chunk pB[chunk][i]; zeros for the disabled
// projections. Both outputs are [3][r W] floats: output i < 3 r W is dA's, the next 3 r W are dB's.
// Block: 64 outputs x 4 quarters of the chunks; thread (o, q) sums its quarter in order, then the
// four quarter sums are added in order: fixed by (rows, W, r) alone.
__global__ __launch_bounds__(256) void final_kernel(int W, int r, int nch, unsigned proj_mask, float s,
                                                    const float* __restrict__ pA, const float* __restrict__ pB,
                                                    float* __restrict__ dA, float* __restrict__ dB) {
  __shared__ float qs[4][64];
  const size_t n = (size_t)3 * r * W;  // (a multiple of 64)
  const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
  const size_t i = (size_t)blockIdx.x * 64 + o;
  const bool isb = i >= n;  // block-uniform
  const size_t e = isb ? i - n : i;
  const int p = (int)(e / ((size_t)r * W));
  const bool on = (proj_mask >> p) & 1u;
  float acc = 0.f;
  if (on) {
    const int cq = (nch + 3) / 4;
    const int ca = q * cq, cb = min(ca + cq, nch);
    const float* src = (isb ? pB : pA) + e;
#pragma unroll 8
    for (int c = ca; c < cb; ++c) acc += src[(size_t)c * n];
  }
  qs[q][o] = acc;
  __syncthreads();
  if (q == 0) {
    float tot = ((qs[0][o] + qs[1][o]) + qs[2][o]) + qs[3][o];
    if (isb) tot *= s;
    (isb ? dB : dA)[e] = on ? tot : 0.f;
  }
}

bool wgrad_shape_ok(int rows, int W, int r) { return rows >= 1 && W >= 64 && W % 64 == 0 && r >= 1 && r <= kMaxRank; }

struct WgradArgs {
  int rows, W, r;
  unsigned pm;
  float s;
  const void *X, *dY;
  const float *mean, *rstd, *gamma, *beta, *A, *B;
  float *dA, *dB;
  Ws w;
  hipStream_t st;
};

template <typename TX, typename TG, int RP>
int wgrad_run(const WgradArgs& a) {
  hipLaunchKernelGGL((rows_kernel<TX, TG, RP>), dim3((unsigned)((a.rows + RT - 1) / RT), 4), dim3(256), 0, a.st, a.rows,
                     a.W, a.r, a.pm, a.s, (const TX*)a.X, a.mean, a.rstd, a.gamma, a.beta, (const TG*)a.dY, a.A, a.B,
                     a.w.P, a.w.dU);
  CLIPK_CHECK_LAUNCH();
  hipLaunchKernelGGL((part_kernel<TX, TG, RP>), dim3((unsigned)(4 * a.W / 64), (unsigned)a.w.nch), dim3(64), 0, a.st,
                     a.rows, a.W, a.r, a.w.ch, a.pm, (const TX*)a.X, a.mean, a.rstd, a.gamma, a.beta,
                     (const TG*)a.dY, (const float*)a.w.P, (const float*)a.w.dU, a.w.pA, a.w.pB);
  CLIPK_CHECK_LAUNCH();
  const size_t n2 = (size_t)6 * a.r * a.W;  // (W % 64 == 0: whole blocks of 64 outputs)
  hipLaunchKernelGGL(final_kernel, dim3((unsigned)(n2 / 64)), dim3(256), 0, a.st, a.W, a.r, a.w.nch, a.pm,
                     a.s, (const float*)a.w.pA, (const float*)a.w.pB, a.dA, a.dB);
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

template <typename TX, typename TG>
int wgrad_rank(const WgradArgs& a) {
  if (a.r == 1) return wgrad_run<TX, TG, 1>(a);
  if (a.r == 2) return wgrad_run<TX, TG, 2>(a);
  if (a.r <= 4) return wgrad_run<TX, TG, 4>(a);
  if (a.r <= 8) return wgrad_run<TX, TG, 8>(a);
  return wgrad_run<TX, TG, 16>(a);
}

template <typename TX>
int wgrad_g(int gd, const WgradArgs& a) {
  if (gd == CLIPK_F32) return wgrad_rank<TX, float>(a);
  if (gd == CLIPK_F16) return wgrad_rank<TX, f16>(a);
  if (gd == CLIPK_BF16) return wgrad_rank<TX, bf16>(a);
  return CLIPK_EDTYPE;
}

}  // namespace

extern "C" int clipk_lora_merge(int W, int layers, int rank, int proj_mask, unsigned layer_mask, float scale,
                                int act_dtype, int grad_dtype, const float* const* w0, const float* A,
                                const float* B, void* const* out, void* const* outT, void* stream) {
  if (!w0 || !A || !B || !out) return CLIPK_EINVAL;
  if (W < 64 || W % 64 || rank < 1 || rank > kMaxRank || layers < 1 || layers > kMaxLayers) return CLIPK_EINVAL;
  if (proj_mask < 0 || proj_mask > 7) return CLIPK_EINVAL;
  MergePtrs ptrs;
  for (int l = 0; l < layers; ++l) {
    if (!w0[l] || !out[l]) return CLIPK_EINVAL;
    if (outT && (outT[l] != nullptr) != (outT[0] != nullptr)) return CLIPK_EINVAL;  // all or none
    ptrs.w0[l] = w0[l];
    ptrs.out[l] = out[l];
    ptrs.outT[l] = outT ? outT[l] : nullptr;
    if (((uintptr_t)ptrs.w0[l] | (uintptr_t)ptrs.out[l] | (uintptr_t)ptrs.outT[l]) & 15) return CLIPK_EINVAL;
  }
  if (((uintptr_t)A | (uintptr_t)B) & 15) return CLIPK_EINVAL;
  // A's rows are read 16 bytes at a time: rows of W floats are 16-byte aligned (W % 64 == 0)
  const dim3 grid((unsigned)(W / MT), (unsigned)(3 * W / MT), (unsigned)layers);
  hipStream_t st = (hipStream_t)stream;
  const unsigned pm = (unsigned)proj_mask;
  if (act_dtype == CLIPK_F32) return merge_launch_g<float>(grad_dtype, grid, st, W, rank, pm, layer_mask, scale, ptrs, A, B);
  if (act_dtype == CLIPK_F16) return merge_launch_g<f16>(grad_dtype, grid, st, W, rank, pm, layer_mask, scale, ptrs, A, B);
  if (act_dtype == CLIPK_BF16) return merge_launch_g<bf16>(grad_dtype, grid, st, W, rank, pm, layer_mask, scale, ptrs, A, B);
  return CLIPK_EDTYPE;
}

extern "C" size_t clipk_lora_wgrad_ws_bytes(int rows, int W, int rank) {
  if (!wgrad_shape_ok(rows, W, rank)) return 0;
  return (carve(nullptr, rows, W, rank).floats * sizeof(float) + 255) / 256 * 256;
}

extern "C" int clipk_lora_wgrad(int x_dtype, int g_dtype, int rows, int W, int rank, int proj_mask, float scale,
                                const void* X, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, const void* dqkv, const float* A, const float* B, float* dA,
                                float* dB, void* ws, size_t ws_bytes, void* stream) {
  if (!X || !mean || !rstd || !gamma || !beta || !dqkv || !A || !B || !dA || !dB || !ws) return CLIPK_EINVAL;
  if (!wgrad_shape_ok(rows, W, rank) || proj_mask < 0 || proj_mask > 7) return CLIPK_EINVAL;
  if (((uintptr_t)X | (uintptr_t)dqkv | (uintptr_t)A | (uintptr_t)B | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)ws) & 15)
    return CLIPK_EINVAL;
  if (ws_bytes < clipk_lora_wgrad_ws_bytes(rows, W, rank)) return CLIPK_EWORKSPACE;
  WgradArgs a;
  a.rows = rows; a.W = W; a.r = rank; a.pm = (unsigned)proj_mask; a.s = scale;
  a.X = X; a.dY = dqkv; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.A = A; a.B = B;
  a.dA = dA; a.dB = dB;
  a.w = carve((float*)ws, rows, W, rank);
  a.st = (hipStream_t)stream;
  if (x_dtype == CLIPK_F32) return wgrad_g<float>(g_dtype, a);
  if (x_dtype == CLIPK_F16) return wgrad_g<f16>(g_dtype, a);
  if (x_dtype == CLIPK_BF16) return wgrad_g<bf16>(g_dtype, a);
  return CLIPK_EDTYPE;
}
