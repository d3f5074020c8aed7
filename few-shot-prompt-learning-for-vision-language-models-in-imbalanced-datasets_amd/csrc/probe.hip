// Linear-probe head (clipk_probe_head, include/clipk.h): nn.Linear on the frozen image features,
// CE / focal, and the gradients of the classifier's weight and bias, from one call.
//
//   u_b = normalize ? feat_b / max(|feat_b|, 1e-12) : feat_b
//   s = scale u w^T + bias        loss = mean_b L(s_b, y_b) (CE or focal, clipk_ce_loss's arithmetic)
//   G = d loss / d s = wgt_b / B (softmax(s_b) - onehot(y_b))
//   d_w = grad_scale scale G^T u  d_bias = grad_scale sum_b G_b     (nothing for feat: frozen encoder)
//
// Three launches, data handed on at kernel boundaries only:
//  1. logits_kernel  s on 32 x 32 tiles of (b, c), the whole of E in one block: fp32 FMA chains over
//                    stages of 32 elements, each stage's sum added to the running one. The blocks
//                    take 1 / |feat_b| from the squares of the feat rows they stage anyway, so
//                    scoring only (labels NULL) is this launch alone.
//  2. rows_kernel    one wave per row: row max, log of the sum of exponentials, the CE / focal row
//                    loss and G. Forward only: one block walks all rows and sums the row losses.
//  3. grad_kernel    d_w on 32 x 32 tiles of (c, e), the sum over b in row order; further blocks of
//                    the same launch: d_bias (one thread per class) and the sum of the row losses.
// Products on the fp32 VALU (the tile of srchead.hip / ntxent.hip), not on MFMA: DESIGN.md, "Probe
// head kernel". No atomics, every sum in an order fixed by (B, C, E): bitwise reproducible.
// Global loads are unconditional on clamped (always in-bounds) indices, with a select for what lies
// outside (ntxent.hip has the reason); 16-byte loads where E % 4 == 0 and the arrays are 16-byte
// aligned, one float at a time otherwise.
#include "common.h"

using namespace clipk;

namespace {

constexpr int KC = 32;      // reduction-dimension elements per LDS stage
constexpr int RS = KC + 4;  // LDS row stride in floats (16-byte aligned rows)
constexpr int T = 32;       // output tile edge: 256 threads x (2 x 2)
constexpr int kMaxB = 512;
constexpr int kFwdWaves = 16;  // waves of the forward-only rows block

struct Ws {
  float *rinv, *rowloss, *S, *G;
  int ldg;  // row stride of G: C rounded up to 4 floats (16-byte rows)
  size_t floats;
};

// base may be null (clipk_probe_head_ws_bytes): only floats is meaningful then. Every part starts
// on a multiple of 4 floats.
Ws carve(float* base, int B, int C) {
  Ws w;
  size_t o = 0;
  auto take = [&](size_t n) {
    float* f = base ? base + o : nullptr;
    o += (n + 3) / 4 * 4;
    return f;
  };
  w.ldg = (C + 3) / 4 * 4;
  w.rinv = take(B);
  w.rowloss = take(B);
  w.S = take((size_t)B * C);
  w.G = take((size_t)B * w.ldg);
  w.floats = o;
  return w;
}

// Elements k .. k + 3 of a row of n floats, zeros from n on. VEC: n % 4 == 0, k % 4 == 0 and the row
// 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ row, int k, int n) {
  f32x4 v;
  if constexpr (VEC) {
    v = *reinterpret_cast<const f32x4*>(row + min(k, n - 4));
    if (k >= n) v = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x = row[min(k + j, n - 1)];
      v[j] = k + j < n ? x : 0.f;
    }
  }
  return v;
}

// Block (it, jt): s[b][c] for the 32 rows from 32 it and the 32 classes from 32 jt. Loader: thread t
// stages elements 4 (t & 7) .. + 3 of row t >> 3 of both operands; thread (tx, ty) owns rows
// ty + 16 m and classes tx + 16 c of the tile.
template <bool VEC>
__global__ __launch_bounds__(256) void logits_kernel(int B, int C, int E, int tc, int normalize, float scale,
                                                     const float* __restrict__ feat, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ S,
                                                     float* __restrict__ rinv) {
  __shared__ CLIPK_LDS_ALIGN float As[T * RS];
  __shared__ CLIPK_LDS_ALIGN float Bs[T * RS];
  __shared__ float rn[T];
  const int t = threadIdx.x;
  const int jt = blockIdx.x % tc, it = blockIdx.x / tc;
  const int tx = t & 15, ty = t >> 4;
  const int lr = t >> 3, lk = (t & 7) * 4;
  const int I0 = it * T, J0 = jt * T;
  const bool va = I0 + lr < B, vb = J0 + lr < C;
  const float* pa = feat + (size_t)min(I0 + lr, B - 1) * E;
  const float* pb = w + (size_t)min(J0 + lr, C - 1) * E;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 ra = load_quad<VEC>(pa, lk, E), rb = load_quad<VEC>(pb, lk, E);
  float tot[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  float ss = 0.f;
  for (int ks = 0; ks < E; ks += KC) {
    *reinterpret_cast<f32x4*>(&As[lr * RS + lk]) = va ? ra : zero;
    *reinterpret_cast<f32x4*>(&Bs[lr * RS + lk]) = vb ? rb : zero;
#pragma unroll
    for (int j = 0; j < 4; ++j) ss = fmaf(ra[j], ra[j], ss);
    __syncthreads();
    if (ks + KC < E) {
      ra = load_quad<VEC>(pa, ks + KC + lk, E);
      rb = load_quad<VEC>(pb, ks + KC + lk, E);
    }
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      f32x4 av[2], bv[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) av[m] = *reinterpret_cast<const f32x4*>(&As[(ty + 16 * m) * RS + kk]);
#pragma unroll
      for (int c = 0; c < 2; ++c) bv[c] = *reinterpret_cast<const f32x4*>(&Bs[(tx + 16 * c) * RS + kk]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[m][c] = fmaf(av[m][e], bv[c][e], acc[m][c]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int c = 0; c < 2; ++c) tot[m][c] += acc[m][c];
    __syncthreads();
  }
  // |feat_b|^2: the 8 loader lanes of a row, each its own stages in order, then the butterfly
  ss = group_sum<8>(ss);
  const float r = normalize ? 1.0f / fmaxf(sqrtf(ss), 1e-12f) : 1.0f;  // F.normalize's clamp
  if ((t & 7) == 0) {
    rn[lr] = r;
    if (rinv && jt == 0 && va) rinv[I0 + lr] = r;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int i = I0 + ty + 16 * m;
    const float sr = scale * rn[ty + 16 * m];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = J0 + tx + 16 * c;
      if (i < B && j < C) S[(size_t)i * C + j] = tot[m][c] * sr + (bias ? bias[j] : 0.f);
    }
  }
}

// One wave, row b: the CE / focal row loss (returned in every lane) and, with g, G's row.
__device__ __forceinline__ float row_wave(int C, int lane, const float* __restrict__ s, int64_t y,
                                          const float* __restrict__ alpha, float gamma, int focal, float inv_b,
                                          float* __restrict__ g) {
  const bool yok = y >= 0 && y < C;
  float mx = -INFINITY, sy = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = s[c];
    mx = fmaxf(mx, v);
    sy += (c == y) ? v : 0.f;  // one lane holds it, the others add zeros
  }
  mx = wave_max(mx);
  sy = wave_sum(sy);
  float es = 0.f;
  for (int c = lane; c < C; c += 64) es += expf(s[c] - mx);
  const float lgs = logf(wave_sum(es));
  // clipk_ce_loss's row terms; a label outside [0, C) was never dereferenced: NaN
  float l, wgt;
  if (!yok) {
    l = wgt = __builtin_nanf("");
  } else {
    const float ce = (mx - sy) + lgs;
    l = ce;
    wgt = 1.f;
    if (focal) {
      focal_terms(ce, expf(-ce), alpha ? alpha[y] : 1.f, gamma, l, wgt);
    }
  }
  if (g) {
    const float cw = wgt * inv_b;
    for (int c = lane; c < C; c += 64) g[c] = cw * (expf((s[c] - mx) - lgs) - (c == y ? 1.f : 0.f));
  }
  return l;
}

// loss[0] = (1/B) sum of the row losses by one wave: lane l sums rows l, l + 64, ... in order, then
// the butterfly.
__device__ __forceinline__ void loss_reduce(int B, int lane, const float* v, float inv_b, float* __restrict__ loss) {
  float s = 0.f;
  for (int i = lane; i < B; i += 64) s += v[i];
  s = wave_sum(s);
  if (lane == 0) loss[0] = s * inv_b;
}

// With gradients: wave w of the grid takes row w.
__global__ __launch_bounds__(256) void rows_kernel(int B, int C, int ldg, const float* __restrict__ S,
                                                   const int64_t* __restrict__ labels,
                                                   const float* __restrict__ alpha, float gamma, int focal,
                                                   float inv_b, float* __restrict__ G, float* __restrict__ rowloss) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float l = row_wave(C, lane, S + (size_t)b * C, labels[b], alpha, gamma, focal, inv_b, G + (size_t)b * ldg);
  if (lane == 0) rowloss[b] = l;
}

// Forward only: one block, wave w takes rows w, w + 16, ...; then the sum of the row losses.
__global__ __launch_bounds__(64 * kFwdWaves) void rows_loss_kernel(int B, int C, const float* __restrict__ S,
                                                                   const int64_t* __restrict__ labels,
                                                                   const float* __restrict__ alpha, float gamma,
                                                                   int focal, float inv_b, float* __restrict__ loss) {
  __shared__ float rl[kMaxB];
  const int lane = threadIdx.x & 63;
  for (int b = threadIdx.x >> 6; b < B; b += kFwdWaves) {
    const float l = row_wave(C, lane, S + (size_t)b * C, labels[b], alpha, gamma, focal, inv_b, nullptr);
    if (lane == 0) rl[b] = l;
  }
  __syncthreads();
  if (threadIdx.x < 64) loss_reduce(B, lane, rl, inv_b, loss);
}

// Blocks [0, nprod): d_w[c][e] = gs sum_b G[b][c] feat[b][e] rinv[b] for the 32 classes from 32 jt
// and the 32 elements from 32 et (gs = grad_scale scale). Loader: thread t stages classes / elements
// 4 (t & 7) .. + 3 of row b = t >> 3 of the stage; thread (tx, ty) owns classes 2 ty, 2 ty + 1 and
// elements 2 tx, 2 tx + 1. Blocks [nprod, nprod + nbias): d_bias, one thread per class, rows in
// order. The last block: the loss.
template <bool VEC>
__global__ __launch_bounds__(256) void grad_kernel(int B, int C, int E, int ldg, int te, int nprod, int nbias,
                                                   float gs, float grad_scale, float inv_b,
                                                   const float* __restrict__ feat, const float* __restrict__ G,
                                                   const float* __restrict__ rinv,
                                                   const float* __restrict__ rowloss, float* __restrict__ loss,
                                                   float* __restrict__ d_w, float* __restrict__ d_bias) {
  const int t = threadIdx.x;
  if ((int)blockIdx.x >= nprod) {
    const int r = blockIdx.x - nprod;
    if (r < nbias) {
      const int c = r * 256 + t;
      const int cc = min(c, C - 1);
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += G[(size_t)b * ldg + cc];
      if (c < C) d_bias[c] = grad_scale * s;
    } else if (t < 64) {
      loss_reduce(B, t, rowloss, inv_b, loss);
    }
    return;
  }
  __shared__ CLIPK_LDS_ALIGN float Gs[KC * RS];
  __shared__ CLIPK_LDS_ALIGN float Us[KC * RS];
  const int et = blockIdx.x % te, jt = blockIdx.x / te;
  const int tx = t & 15, ty = t >> 4;
  const int lr = t >> 3, lq = (t & 7) * 4;
  const int J0 = jt * T, E0 = et * T;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 rg, ru;
  float rr;
  auto fetch = [&](int b0) {
    const int b = min(b0 + lr, B - 1);
    rg = load_quad<true>(G + (size_t)b * ldg, J0 + lq, ldg);  // (the padding columns feed classes >= C only)
    ru = load_quad<VEC>(feat + (size_t)b * E, E0 + lq, E);
    rr = rinv[b];
  };
  fetch(0);
  float tot[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int b0 = 0; b0 < B; b0 += KC) {
    const bool ok = b0 + lr < B;
    *reinterpret_cast<f32x4*>(&Gs[lr * RS + lq]) = ok ? rg : zero;
    *reinterpret_cast<f32x4*>(&Us[lr * RS + lq]) = ok ? ru * rr : zero;
    __syncthreads();
    if (b0 + KC < B) fetch(b0 + KC);
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const f32x2 a = *reinterpret_cast<const f32x2*>(&Gs[k * RS + 2 * ty]);
      const f32x2 u = *reinterpret_cast<const f32x2*>(&Us[k * RS + 2 * tx]);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[m][c] = fmaf(a[m], u[c], acc[m][c]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int c = 0; c < 2; ++c) tot[m][c] += acc[m][c];
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int j = J0 + 2 * ty + m;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int e = E0 + 2 * tx + c;
      if (j < C && e < E) d_w[(size_t)j * E + e] = gs * tot[m][c];
    }
  }
}

bool shape_ok(int B, int C, int E) { return B >= 1 && B <= kMaxB && C >= 1 && E >= 1; }

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" size_t clipk_probe_head_ws_bytes(int B, int C, int E) {
  if (!shape_ok(B, C, E)) return 0;
  return (carve(nullptr, B, C).floats * sizeof(float) + 255) / 256 * 256;
}

extern "C" int clipk_probe_head(int B, int C, int E, const float* feat, const float* w, const float* bias,
                                const int64_t* labels, const float* alpha, float gamma, int focal, int normalize,
                                float scale, float grad_scale, float* loss, float* logits, float* d_w,
                                float* d_bias, void* ws, void* stream) {
  if (!feat || !w) return CLIPK_EINVAL;
  if (!labels) {
    if (!logits || loss || d_w || d_bias) return CLIPK_EINVAL;
  } else {
    if (!loss || !ws || (uintptr_t)ws % 16) return CLIPK_EINVAL;
    if ((d_bias != nullptr) != (d_w != nullptr && bias != nullptr)) return CLIPK_EINVAL;
    if (focal && !(gamma >= 0.f)) return CLIPK_EINVAL;
  }
  if (!(scale > 0.f)) return CLIPK_EINVAL;
  if (!shape_ok(B, C, E)) return CLIPK_ESHAPE;
  const int tb = (B + T - 1) / T, tc = (C + T - 1) / T, te = (E + T - 1) / T;
  const int nbias = d_bias ? (C + 255) / 256 : 0;
  if ((long)tb * tc > 0x7fffffffL || (long)tc * te + nbias + 1 > 0x7fffffffL) return CLIPK_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  const Ws p = carve(labels ? (float*)ws : nullptr, B, C);
  float* S = logits ? logits : p.S;
  const bool vec = E % 4 == 0 && aligned16(feat) && aligned16(w);
#define CLIPK_PROBE_LOGITS(VEC)                                                                                \
  hipLaunchKernelGGL(logits_kernel<VEC>, dim3((unsigned)(tb * tc)), dim3(256), 0, st, B, C, E, tc, normalize, \
                     scale, feat, w, bias, S, p.rinv)
  if (vec) CLIPK_PROBE_LOGITS(true);
  else CLIPK_PROBE_LOGITS(false);
#undef CLIPK_PROBE_LOGITS
  CLIPK_CHECK_LAUNCH();
  if (!labels) return CLIPK_OK;
  const float inv_b = 1.0f / (float)B;
  if (!d_w) {
    hipLaunchKernelGGL(rows_loss_kernel, dim3(1), dim3(64 * kFwdWaves), 0, st, B, C, S, labels, alpha, gamma, focal,
                       inv_b, loss);
    CLIPK_CHECK_LAUNCH();
    return CLIPK_OK;
  }
  hipLaunchKernelGGL(rows_kernel, dim3((B + 3) / 4), dim3(256), 0, st, B, C, p.ldg, S, labels, alpha, gamma, focal,
                     inv_b, p.G, p.rowloss);
  CLIPK_CHECK_LAUNCH();
  const int nprod = tc * te;
  const float gs = grad_scale * scale;
#define CLIPK_PROBE_GRAD(VEC)                                                                                       \
  hipLaunchKernelGGL(grad_kernel<VEC>, dim3((unsigned)(nprod + nbias + 1)), dim3(256), 0, st, B, C, E, p.ldg, te,   \
                     nprod, nbias, gs, grad_scale, inv_b, feat, p.G, p.rinv, p.rowloss, loss, d_w, d_bias)
  if (E % 4 == 0 && aligned16(feat)) CLIPK_PROBE_GRAD(true);
  else CLIPK_PROBE_GRAD(false);
#undef CLIPK_PROBE_GRAD
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}
