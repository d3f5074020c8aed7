// Mixup (mixup_data / mixup_criterion, PromptSRC/trainers/independentVL.py:435-460):
//   clipk_mixup_images  out[b] = w0 * x[b] + w1 * x[perm[b]] (and y_b[b] = labels[perm[b]])
//   clipk_ce_loss_mix   lam * L(logits, y_a) + (1 - lam) * L(logits, y_b), forward and gradient
// (include/clipk.h).
//
// mixup_images is HBM-bound (two reads and one write per element): every thread loads all of its
// 16-byte pieces of both rows before the first store, UNROLL of them, so a wave keeps 2 * UNROLL
// KiB in flight. The two products are rounded to fp32 separately and then added, which is torch's
// lam * x + (1 - lam) * x[perm] bit for bit when w0 = (float)lam and w1 = (float)(1.0 - lam):
// mul_add_rn below, under "fp contract(off)" -- hipcc's __fmul_rn / __fadd_rn are plain * and +,
// which the default -ffp-contract=fast fuses into v_pk_fma_f32 (one rounding fewer). Rows start
// 16-byte aligned only when n_per % 4 == 0 and the base pointers are; every other case takes the
// one-float path.
//
// ce_loss_mix is the two-target form of ce_loss_reduce_kernel (prompt.hip), the same arithmetic
// per row: one max pass and one sum-of-exponentials pass serve both targets, and the gradient
// pass forms p_c once. One block of MIXW = 8 waves; wave w takes rows w, w + 8, ...; one thread
// sums the row losses in row order. No atomics: results are bitwise reproducible. Rows of C <= 64 * ROWQ (1,024)
// classes are loaded once, ROWQ logits per lane, all loads issued before the first use: the three
// passes then run from registers in the same per-lane order (bitwise the looping form, which
// longer rows keep). The looping form pays one L2 round trip per 64 logits and pass: 48 dependent
// round trips per row at C = 1000, which was the whole 56 us of the first build at [32, 1000].
#include "common.h"

using namespace clipk;

namespace {

constexpr int UNROLL = 4;  // pieces per thread of the image mix

// round(round(w0 * a) + round(w1 * b)): never contracted into an FMA
__device__ __forceinline__ float mul_add_rn(float w0, float a, float w1, float b) {
#pragma clang fp contract(off)
  const float pa = w0 * a;
  const float pb = w1 * b;
  return pa + pb;
}

// V = f32x4 (n = n_per / 4 pieces per row) or float (n = n_per)
template <typename V>
__global__ __launch_bounds__(256) void mixup_images_kernel(int B, long n, const V* __restrict__ x,
                                                           const int* __restrict__ perm,
                                                           const int64_t* __restrict__ labels,
                                                           int64_t* __restrict__ y_b, float w0, float w1,
                                                           V* __restrict__ out) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    int p = perm[b];
    if (p < 0 || p >= B) p = b;  // never dereferenced out of range: the row mixes with itself
    if (y_b && blockIdx.x == 0 && threadIdx.x == 0) y_b[b] = labels[p];
    const V* xa = x + (size_t)b * n;
    const V* xb = x + (size_t)p * n;
    V* o = out + (size_t)b * n;
    const long i0 = (long)blockIdx.x * (256 * UNROLL) + threadIdx.x;
    V va[UNROLL], vb[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long i = i0 + u * 256;
      if (i < n) { va[u] = xa[i]; vb[u] = xb[i]; }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long i = i0 + u * 256;
      if (i < n) {
        if constexpr (sizeof(V) == 16) {
          V r;
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = mul_add_rn(w0, va[u][k], w1, vb[u][k]);
          o[i] = r;
        } else {
          o[i] = mul_add_rn(w0, va[u], w1, vb[u]);
        }
      }
    }
  }
}

// One target's loss and gradient weight from the row's logsumexp (ce_loss_reduce_kernel's
// arithmetic). A label outside [0, C) is not dereferenced: NaN loss and weight.
__device__ __forceinline__ void target_terms(const float* __restrict__ z, int C, int64_t y, float lse,
                                             const float* __restrict__ alpha, float gamma, int focal, float& l,
                                             float& wgt) {
  if (y < 0 || y >= C) {
    l = wgt = __builtin_nanf("");
    return;
  }
  const float ce = lse - z[y];
  l = ce;
  wgt = 1.f;
  if (focal) {
    focal_terms(ce, __expf(-ce), alpha ? alpha[y] : 1.f, gamma, l, wgt);
  }
}

constexpr int ROWQ = 16;  // logits per lane of a row held in registers
constexpr int MIXW = 8;   // waves of the one block (rows in flight)

template <bool CACHED>
__global__ __launch_bounds__(64 * MIXW) void ce_loss_mix_kernel(int B, int C, const float* __restrict__ logits,
                                                          const int64_t* __restrict__ y_a,
                                                          const int64_t* __restrict__ y_b, float lam,
                                                          const float* __restrict__ alpha, float gamma, int focal,
                                                          float grad_scale, int mean, float* __restrict__ row_loss,
                                                          float* __restrict__ loss, float* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float lam1 = 1.f - lam;
  for (int b = wv; b < B; b += MIXW) {
    const float* z = logits + (size_t)b * C;
    const int64_t ya = y_a[b], yb = y_b[b];
    float zc[ROWQ];
    float mx = -INFINITY, se = 0.f;
    if constexpr (CACHED) {
      // unconditional loads on a clamped index, then a select: all ROWQ in flight at once
#pragma unroll
      for (int q = 0; q < ROWQ; ++q) {
        const int c = lane + 64 * q;
        const float v = z[c < C ? c : C - 1];
        zc[q] = c < C ? v : -INFINITY;
      }
#pragma unroll
      for (int q = 0; q < ROWQ; ++q) mx = fmaxf(mx, zc[q]);
      mx = wave_max(mx);
#pragma unroll
      for (int q = 0; q < ROWQ; ++q)
        if (lane + 64 * q < C) se += __expf(zc[q] - mx);
    } else {
      for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
      mx = wave_max(mx);
      for (int c = lane; c < C; c += 64) se += __expf(z[c] - mx);
    }
    se = wave_sum(se);
    const float lse = mx + __logf(se);
    float la, wa, lb, wb;
    target_terms(z, C, ya, lse, alpha, gamma, focal, la, wa);
    target_terms(z, C, yb, lse, alpha, gamma, focal, lb, wb);
    if (lane == 0) {
      row_loss[b] = la;
      row_loss[B + b] = lb;
    }
    if (dlogits) {
      const float ca = lam * (grad_scale * wa), cb = lam1 * (grad_scale * wb);
      // (a row with y_a == y_b: both terms land on column y_a)
      if constexpr (CACHED) {
#pragma unroll
        for (int q = 0; q < ROWQ; ++q) {
          const int c = lane + 64 * q;
          const float pc = __expf(zc[q] - lse);
          if (c < C)
            dlogits[(size_t)b * C + c] = ca * (pc - (c == ya ? 1.f : 0.f)) + cb * (pc - (c == yb ? 1.f : 0.f));
        }
      } else {
        for (int c = lane; c < C; c += 64) {
          const float pc = __expf(z[c] - lse);
          dlogits[(size_t)b * C + c] = ca * (pc - (c == ya ? 1.f : 0.f)) + cb * (pc - (c == yb ? 1.f : 0.f));
        }
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    float sa = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) sa += row_loss[b];
    for (int b = 0; b < B; ++b) sb += row_loss[B + b];
    if (mean) {  // (torch's mean: the sum times 1 / B)
      sa *= 1.0f / (float)B;
      sb *= 1.0f / (float)B;
    }
    // the trainer's lam * L_a + (1 - lam) * L_b: two rounded products, then the sum
    loss[0] = mul_add_rn(lam, sa, lam1, sb);
  }
}

}  // namespace

extern "C" int clipk_mixup_images(int B, long n_per, const float* x, const int* perm, const int64_t* labels,
                                  int64_t* y_b, float w0, float w1, float* out, void* stream) {
  if (B == 0) return CLIPK_OK;
  if (B < 0 || n_per <= 0) return CLIPK_ESHAPE;
  if (!x || !perm || !out) return CLIPK_EINVAL;
  if ((labels == nullptr) != (y_b == nullptr)) return CLIPK_EINVAL;
  const uintptr_t xs = (uintptr_t)x, os = (uintptr_t)out;
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)n_per * sizeof(float);
  // out overlapping x: a row would be read after another block has overwritten it
  if (os < xs + bytes && xs < os + bytes) return CLIPK_EINVAL;
  const int gy = B < 65535 ? B : 65535;
  const bool vec = n_per % 4 == 0 && xs % 16 == 0 && os % 16 == 0;
  const long n = vec ? n_per / 4 : n_per;
  const long gx = (n + 256 * UNROLL - 1) / (256 * UNROLL);
  if (gx > 0x7fffffffL) return CLIPK_ESHAPE;
  if (vec)
    hipLaunchKernelGGL(mixup_images_kernel<f32x4>, dim3((unsigned)gx, gy), dim3(256), 0, (hipStream_t)stream, B, n,
                       reinterpret_cast<const f32x4*>(x), perm, labels, y_b, w0, w1, reinterpret_cast<f32x4*>(out));
  else
    hipLaunchKernelGGL(mixup_images_kernel<float>, dim3((unsigned)gx, gy), dim3(256), 0, (hipStream_t)stream, B, n, x,
                       perm, labels, y_b, w0, w1, out);
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

extern "C" int clipk_ce_loss_mix(int B, int C, const float* logits, const int64_t* y_a, const int64_t* y_b,
                                 float lam, const float* alpha, float gamma, int focal, float grad_scale,
                                 int reduction, float* row_loss, float* loss, float* dlogits, void* stream) {
  if (!logits || !y_a || !y_b || !row_loss || !loss) return CLIPK_EINVAL;
  if (reduction != 1 && reduction != 2) return CLIPK_EINVAL;
  if (focal && !(gamma >= 0.f)) return CLIPK_EINVAL;
  if (B <= 0 || C <= 0) return CLIPK_ESHAPE;
  const int mean = reduction == 1 ? 1 : 0;
  if (C <= 64 * ROWQ)
    hipLaunchKernelGGL(ce_loss_mix_kernel<true>, dim3(1), dim3(64 * MIXW), 0, (hipStream_t)stream, B, C, logits, y_a,
                       y_b, lam, alpha, gamma, focal, grad_scale, mean, row_loss, loss, dlogits);
  else
    hipLaunchKernelGGL(ce_loss_mix_kernel<false>, dim3(1), dim3(64 * MIXW), 0, (hipStream_t)stream, B, C, logits, y_a,
                       y_b, lam, alpha, gamma, focal, grad_scale, mean, row_loss, loss, dlogits);
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}
