// Image preprocessing on the GPU: Pillow-exact bicubic resampling (two separable passes,
// 22-bit fixed-point coefficients, uint8 rounding + clipping after each pass) over a crop
// window, horizontal flip, and torchvision ToTensor + Normalize in fp32.
// Colour stage (clipk_image_color, below): torchvision ColorJitter / RandomGrayscale on the
// resampled uint8 pixels, Pillow-exact, one workgroup per image (arithmetic in color_ops.h).
// clipk_image_color_blur: the same launch followed by Pillow's GaussianBlur on the image.
//
// Replaces the Dassl/torchvision PIL transforms (Dassl.pytorch/dassl/data/transforms/
// transforms.py:206-354: Resize + CenterCrop for test, RandomResizedCrop + flip for train)
// that run per image on the host. The coefficient tables (Pillow libImaging/Resample.c
// precompute_coeffs + normalize_coeffs_8bpc) are built on the host in float64
// (fsp_amd/data/preprocess.py), or on the device by resample_tables_kernel (clipk_resample_tables;
// arithmetic in resample_ops.h, the same integers); these kernels do the integer work.
// HBM/latency-bound: each output pixel reads ~ksize source pixels per pass.
// clipk_image_resample_at: the same kernels on images addressed absolutely (an image bank).
#include <string.h>

#include "common.h"
#include "color_ops.h"
#include "resample_ops.h"

namespace clipk {

constexpr int kPrecBits = resample::kPrecisionBits;  // Pillow PRECISION_BITS: one constant for the tables and the kernels

__device__ __forceinline__ int clip8(int s) {
  const int v = s >> kPrecBits;  // arithmetic shift, as Pillow's lookup index
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// desc (int64 x 16 per image): 0 src byte offset, 1 source row stride (pixels), 2 window
// left, 3 source row of temp row 0, 4 S, 5 flip, 6 h-table offset, 7 h ksize, 8 v-table
// offset, 9 v ksize, 10 temp byte offset, 11 temp rows, 12 source rows.
// h/v table rows: (first tap, taps used, ksize int32 coefficients).
__global__ __launch_bounds__(256) void resample_h_kernel(int B, int S, int rows_max, const uint8_t* __restrict__ src,
                                                         const long long* __restrict__ desc,
                                                         const int* __restrict__ tab, uint8_t* __restrict__ tmp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)rows_max * S;
  if (i >= per * B) return;
  const int b = (int)(i / per);
  const int r = (int)((i % per) / S), x = (int)(i % S);
  const long long* d = desc + (size_t)b * 16;
  if (r >= (int)d[11]) return;
  const int ks = (int)d[7];
  const int* row = tab + d[6] + (size_t)x * (2 + ks);
  const int xmin = row[0], n = row[1];
  const uint8_t* p = src + d[0] + ((size_t)(d[3] + r) * d[1] + d[2] + xmin) * 3;
  int s0 = 1 << (kPrecBits - 1), s1 = s0, s2 = s0;
  for (int k = 0; k < n; ++k) {
    const int w = row[2 + k];
    s0 += (int)p[3 * k] * w;
    s1 += (int)p[3 * k + 1] * w;
    s2 += (int)p[3 * k + 2] * w;
  }
  uint8_t* o = tmp + d[10] + ((size_t)r * S + x) * 3;
  o[0] = (uint8_t)clip8(s0);
  o[1] = (uint8_t)clip8(s1);
  o[2] = (uint8_t)clip8(s2);
}

template <bool U8>
__global__ __launch_bounds__(256) void resample_v_kernel(int B, int S, const long long* __restrict__ desc,
                                                         const int* __restrict__ tab, const uint8_t* __restrict__ tmp,
                                                         const float* __restrict__ mean, const float* __restrict__ stdv,
                                                         void* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)S * S;
  if (i >= per * B) return;
  const int b = (int)(i / per);
  const int y = (int)((i % per) / S), x = (int)(i % S);
  const long long* d = desc + (size_t)b * 16;
  const int ks = (int)d[9];
  const int* row = tab + d[8] + (size_t)y * (2 + ks);
  const int ymin = row[0], n = row[1];
  const uint8_t* t = tmp + d[10] + ((size_t)ymin * S + x) * 3;
  int s[3] = {1 << (kPrecBits - 1), 1 << (kPrecBits - 1), 1 << (kPrecBits - 1)};
  for (int k = 0; k < n; ++k) {
    const int w = row[2 + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += (int)t[(size_t)k * S * 3 + c] * w;
  }
  const int xo = d[5] ? S - 1 - x : x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = clip8(s[c]);
    const size_t oi = (((size_t)b * 3 + c) * S + y) * S + xo;
    if constexpr (U8) {
      ((uint8_t*)out)[oi] = (uint8_t)v;
    } else {
      const float f = (float)v / 255.0f;          // ToTensor: float().div(255)
      ((float*)out)[oi] = (f - mean[c]) / stdv[c];  // Normalize: sub_(mean).div_(std)
    }
  }
}

// ---- coefficient tables (clipk_resample_tables) ----------------------------------------------
// One thread per table row: B images x (S h rows, then S v rows). A row's sum runs over its taps
// in tap order inside the thread (no reduction across lanes: the order is part of the result),
// and its taps are looped over, never held in registers (ksize has no bound). Every write lies in
// the row's own 2 + ksize ints at the offset and stride the host laid out.
// params (int64 x CLIPK_RESAMPLE_PARAMS per image): include/clipk.h.
__global__ __launch_bounds__(256) void resample_tables_kernel(int B, int S, const long long* __restrict__ params,
                                                              int* __restrict__ tab) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * 2 * S) return;
  const int b = (int)(i / (2 * S));
  const int v = (int)((i / S) & 1), r = (int)(i % S);
  const long long* p = params + (size_t)b * CLIPK_RESAMPLE_PARAMS + (v ? 5 : 0);
  if (r >= (int)params[(size_t)b * CLIPK_RESAMPLE_PARAMS + 10]) return;
  const int ks = (int)p[4];
  const resample::Axis a = resample::make_axis((int)p[0], (int)p[1]);
  const int rel = v ? (int)params[(size_t)b * CLIPK_RESAMPLE_PARAMS + 11] : 0;
  resample::table_row(a, (int)p[2] + r, rel, ks, tab + p[3] + (size_t)r * (2 + ks));
}

// ---- colour stage (clipk_image_color) -------------------------------------------------------
// One workgroup per image. Every lane owns the same groups of 4 consecutive pixels (group index
// = lane, lane + 1024, ...) from the load to the epilogue, so the per-pixel ops of a program need
// no barrier between them; CONTRAST, the one op that needs the whole image, takes its mean L from
// an integer block reduction (order-independent) of the image as the ops before it left it.
// LDS form: the three planes live in LDS (plane stride rounded up to 4 pixels, so a group is one
// aligned dword per plane). In-place form (3 * S * S bytes do not fit): the same loop on the
// caller's uint8 buffer. Groups that are not a whole aligned dword -- the tail of a plane when
// S * S % 4 != 0, and any group of a misaligned plane in global memory -- move byte by byte.
// Blur (descriptors of CLIPK_COLORBLUR_DESC ints, r >= 0; uniform over the workgroup): after the
// program, between two barriers, the lanes give up their pixels and take lines instead -- lane l
// the row l % S of plane l / S for the three box passes along x (one lane keeps its row, so no
// barrier between them), a barrier, then the column l % S for the three along y. A pass runs in
// place (color::box_line: a sliding window, the overwritten inputs in registers), so the image
// needs no second copy. An image with r = -1 skips all of it: the barriers too.
constexpr int kColorThreads = 1024;
constexpr int kColorLdsBytes = 3 * 224 * 224;  // 150,528 B of the CU's 160 KiB; the rest: reduction

__device__ __forceinline__ uint32_t px_load4(const uint8_t* p, int i, int n) {
  if (i + 4 <= n && (((uintptr_t)(p + i)) & 3) == 0) return *reinterpret_cast<const uint32_t*>(p + i);
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k)
    if (i + k < n) v |= (uint32_t)p[i + k] << (8 * k);
  return v;
}

__device__ __forceinline__ void px_store4(uint8_t* p, int i, int n, uint32_t v) {
  if (i + 4 <= n && (((uintptr_t)(p + i)) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p + i) = v;
    return;
  }
  for (int k = 0; k < 4; ++k)
    if (i + k < n) p[i + k] = (uint8_t)(v >> (8 * k));
}

// sum over the block of v (every lane gets it); red: one 64-bit slot per wave in LDS
__device__ __forceinline__ unsigned long long color_block_sum(unsigned v, unsigned long long* red) {
  unsigned long long w = v;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) w += __shfl_xor(w, o, 64);
  __syncthreads();  // red may still be read from an earlier CONTRAST
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  unsigned long long t = 0;
  for (int k = 0; k < kColorThreads / 64; ++k) t += red[k];
  return t;
}

template <bool LDS>
__global__ __launch_bounds__(kColorThreads) void color_kernel(int S, uint8_t* __restrict__ pix,
                                                              const int* __restrict__ prog, int desc,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ stdv, int out_u8,
                                                              void* __restrict__ out) {
  __shared__ uint32_t s_img[LDS ? kColorLdsBytes / 4 : 1];
  __shared__ unsigned long long s_red[kColorThreads / 64];
  const int b = blockIdx.x;
  const int n = S * S, ng = (n + 3) / 4;
  uint8_t* src = pix + (size_t)b * 3 * n;
  const int P = LDS ? ng * 4 : n;  // plane stride of the working copy
  uint8_t* img = LDS ? reinterpret_cast<uint8_t*>(s_img) : src;
  const int* pr = prog + (size_t)b * desc;  // desc ints per image: CLIPK_COLOR_DESC, or with the blur
  const int nops = pr[0];
  const int blur_r = desc == CLIPK_COLORBLUR_DESC ? pr[CLIPK_COLOR_DESC] : -1;

  if (LDS) {
    for (int g = threadIdx.x; g < ng; g += kColorThreads)
      for (int c = 0; c < 3; ++c) px_store4(img + c * P, 4 * g, n, px_load4(src + (size_t)c * n, 4 * g, n));
  }

  for (int k = 0; k < nops; ++k) {
    const int op = pr[1 + k];
    const int ip = pr[1 + CLIPK_COLOR_MAX_OPS + k];
    const float f = __int_as_float(ip);
    int d = 0;  // CONTRAST: the image's mean L, int(sum / count + 0.5)
    if (op == CLIPK_COLOR_CONTRAST) {
      unsigned part = 0;
      for (int g = threadIdx.x; g < ng; g += kColorThreads) {
        const uint32_t r4 = px_load4(img, 4 * g, n), g4 = px_load4(img + P, 4 * g, n),
                       b4 = px_load4(img + 2 * P, 4 * g, n);
        for (int j = 0; j < 4; ++j)
          if (4 * g + j < n)
            part += (unsigned)color::luma((r4 >> (8 * j)) & 255, (g4 >> (8 * j)) & 255, (b4 >> (8 * j)) & 255);
      }
      const unsigned long long sum = color_block_sum(part, s_red);
      d = (int)((2 * sum + (unsigned long long)n) / (2 * (unsigned long long)n));
    }
    for (int g = threadIdx.x; g < ng; g += kColorThreads) {
      const uint32_t r4 = px_load4(img, 4 * g, n), g4 = px_load4(img + P, 4 * g, n),
                     b4 = px_load4(img + 2 * P, 4 * g, n);
      uint32_t ro = 0, go = 0, bo = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int r = (r4 >> (8 * j)) & 255, gg = (g4 >> (8 * j)) & 255, bb = (b4 >> (8 * j)) & 255;
        switch (op) {  // uniform over the block
          case CLIPK_COLOR_BRIGHTNESS:
          case CLIPK_COLOR_CONTRAST:
            r = color::blend(d, r, f), gg = color::blend(d, gg, f), bb = color::blend(d, bb, f);
            break;
          case CLIPK_COLOR_SATURATION: {
            const int l = color::luma(r, gg, bb);
            r = color::blend(l, r, f), gg = color::blend(l, gg, f), bb = color::blend(l, bb, f);
            break;
          }
          case CLIPK_COLOR_HUE:
            color::hue_shift(r, gg, bb, ip);
            break;
          default:  // CLIPK_COLOR_GRAYSCALE (the host admits no other code)
            r = gg = bb = color::luma(r, gg, bb);
            break;
        }
        ro |= (uint32_t)r << (8 * j), go |= (uint32_t)gg << (8 * j), bo |= (uint32_t)bb << (8 * j);
      }
      px_store4(img, 4 * g, n, ro);
      px_store4(img + P, 4 * g, n, go);
      px_store4(img + 2 * P, 4 * g, n, bo);
    }
  }

  if (blur_r >= 0) {
    const uint32_t ww = (uint32_t)pr[CLIPK_COLOR_DESC + 1], fw = (uint32_t)pr[CLIPK_COLOR_DESC + 2];
    __syncthreads();  // every lane's pixels are in img
    for (int l = threadIdx.x; l < 3 * S; l += kColorThreads) {
      uint8_t* row = img + (size_t)(l / S) * P + (size_t)(l % S) * S;
      for (int pass = 0; pass < 3; ++pass) color::box_line(row, S, 1, blur_r, ww, fw);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < 3 * S; l += kColorThreads) {
      uint8_t* col = img + (size_t)(l / S) * P + l % S;
      for (int pass = 0; pass < 3; ++pass) color::box_line(col, S, S, blur_r, ww, fw);
    }
    __syncthreads();
  }

  for (int g = threadIdx.x; g < ng; g += kColorThreads) {
    const int i = 4 * g;
    for (int c = 0; c < 3; ++c) {
      const uint32_t v4 = px_load4(img + c * P, i, n);
      const size_t o = ((size_t)b * 3 + c) * n;
      if (out_u8) {
        px_store4((uint8_t*)out + o, i, n, v4);
      } else {
        float* of = (float*)out + o;
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t = (float)((v4 >> (8 * j)) & 255) / 255.0f;  // ToTensor: float().div(255)
          w[j] = (t - mean[c]) / stdv[c];                           // Normalize: sub_(mean).div_(std)
        }
        if (i + 4 <= n && (((uintptr_t)(of + i)) & 15) == 0) {
          store4(of + i, w[0], w[1], w[2], w[3]);
        } else {
          for (int j = 0; j < 4; ++j)
            if (i + j < n) of[i + j] = w[j];
        }
      }
    }
  }
}

}  // namespace clipk

using namespace clipk;

// src + desc[0] is an image's first byte: the packed upload and its offsets (clipk_image_resample),
// or null and absolute addresses (clipk_image_resample_at).
static int resample_launch(int B, int S, int rows_max, const void* src, const long long* desc, const int* tables,
                           void* tmp, const float* mean, const float* stdv, int out_uint8, void* out,
                           void* stream) {
  if (!desc || !tables || !tmp || !out || (!out_uint8 && (!mean || !stdv))) return CLIPK_EINVAL;
  if (B < 0 || S <= 0 || rows_max <= 0) return CLIPK_ESHAPE;
  if (B == 0) return CLIPK_OK;
  hipStream_t st = (hipStream_t)stream;
  const long long nh = (long long)B * rows_max * S, nv = (long long)B * S * S;
  hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, B, S, rows_max,
                     (const uint8_t*)src, desc, tables, (uint8_t*)tmp);
  CLIPK_CHECK_LAUNCH();
  if (out_uint8)
    hipLaunchKernelGGL(resample_v_kernel<true>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, B, S, desc,
                       tables, (const uint8_t*)tmp, mean, stdv, out);
  else
    hipLaunchKernelGGL(resample_v_kernel<false>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, B, S, desc,
                       tables, (const uint8_t*)tmp, mean, stdv, out);
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

extern "C" int clipk_image_resample(int B, int S, int rows_max, const void* src, const long long* desc,
                                    const int* tables, void* tmp, const float* mean, const float* stdv,
                                    int out_uint8, void* out, void* stream) {
  if (!src) return CLIPK_EINVAL;
  return resample_launch(B, S, rows_max, src, desc, tables, tmp, mean, stdv, out_uint8, out, stream);
}

extern "C" int clipk_image_resample_at(int B, int S, int rows_max, const long long* desc, const int* tables,
                                       void* tmp, const float* mean, const float* stdv, int out_uint8, void* out,
                                       void* stream) {
  return resample_launch(B, S, rows_max, nullptr, desc, tables, tmp, mean, stdv, out_uint8, out, stream);
}

extern "C" int clipk_resample_tables(int B, int S, const long long* params, int* tables, void* stream) {
  if (!params || !tables) return CLIPK_EINVAL;
  if (B < 0 || S <= 0) return CLIPK_ESHAPE;
  if (B == 0) return CLIPK_OK;
  const long long n = (long long)B * 2 * S;
  hipLaunchKernelGGL(resample_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B,
                     S, params, tables);
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

// The host twin: the same header functions in a plain loop, on host pointers; checks every record
// before it writes anything.
extern "C" int clipk_resample_tables_host(int B, int S, const long long* params, int* tables, void* stream) {
  (void)stream;
  if (!params || !tables) return CLIPK_EINVAL;
  if (B < 0 || S <= 0) return CLIPK_ESHAPE;
  for (int b = 0; b < B; ++b) {
    const long long* q = params + (size_t)b * CLIPK_RESAMPLE_PARAMS;
    if (q[10] < 1 || q[10] > S) return CLIPK_ESHAPE;
    for (int v = 0; v < 2; ++v) {
      const long long* p = q + (v ? 5 : 0);
      if (p[0] < 1 || p[0] > INT32_MAX || p[1] < 1 || p[1] > INT32_MAX || p[2] < 0 || p[2] + q[10] > p[1] || p[3] < 0)
        return CLIPK_ESHAPE;
      if (p[4] != resample::make_axis((int)p[0], (int)p[1]).ksize) return CLIPK_ESHAPE;
    }
  }
  for (int b = 0; b < B; ++b) {
    const long long* q = params + (size_t)b * CLIPK_RESAMPLE_PARAMS;
    for (int v = 0; v < 2; ++v) {
      const long long* p = q + (v ? 5 : 0);
      const int ks = (int)p[4];
      const resample::Axis a = resample::make_axis((int)p[0], (int)p[1]);
      for (int r = 0; r < (int)q[10]; ++r)
        resample::table_row(a, (int)p[2] + r, v ? (int)q[11] : 0, ks, tables + p[3] + (size_t)r * (2 + ks));
    }
  }
  return CLIPK_OK;
}

// The host checks of both colour entries (nothing is launched or copied before they pass) and the
// launch; desc: ints per image, CLIPK_COLOR_DESC or CLIPK_COLORBLUR_DESC.
static int color_launch(int B, int S, int desc, void* pix, const int* prog, int* prog_dev, const float* mean,
                        const float* stdv, int out_uint8, void* out, void* stream) {
  if (!pix || !prog || !prog_dev || !out || out == pix || (!out_uint8 && (!mean || !stdv))) return CLIPK_EINVAL;
  if (B < 0 || S <= 0 || S > 4096) return CLIPK_ESHAPE;
  for (int b = 0; b < B; ++b) {
    const int* p = prog + (size_t)b * desc;
    if (p[0] < 0 || p[0] > CLIPK_COLOR_MAX_OPS) return CLIPK_ESHAPE;
    for (int k = 0; k < p[0]; ++k) {
      const int op = p[1 + k], ip = p[1 + CLIPK_COLOR_MAX_OPS + k];
      if (op == CLIPK_COLOR_BRIGHTNESS || op == CLIPK_COLOR_CONTRAST || op == CLIPK_COLOR_SATURATION) {
        float f;
        memcpy(&f, &ip, sizeof f);
        if (!(f >= 0.0f) || f > 3.0e38f) return CLIPK_EINVAL;  // negative, NaN or inf
      } else if (op == CLIPK_COLOR_HUE) {
        if (ip < 0 || ip > 255) return CLIPK_EINVAL;
      } else if (op != CLIPK_COLOR_GRAYSCALE) {
        return CLIPK_EINVAL;
      }
    }
    if (desc == CLIPK_COLORBLUR_DESC) {
      const long long r = p[CLIPK_COLOR_DESC], ww = p[CLIPK_COLOR_DESC + 1], fw = p[CLIPK_COLOR_DESC + 2];
      if (r < -1 || r > CLIPK_BLUR_MAX_RADIUS) return CLIPK_EINVAL;
      if (r >= 0 && (ww <= 0 || ww > (1ll << 24) || fw < 0 || (2 * r + 1) * ww + 2 * fw > (1ll << 24)))
        return CLIPK_EINVAL;
    }
  }
  if (B == 0) return CLIPK_OK;
  hipStream_t st = (hipStream_t)stream;
  // pageable host memory: staged before the call returns, so prog may be freed or reused at once
  hipError_t e = hipMemcpyAsync(prog_dev, prog, (size_t)B * desc * sizeof(int), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  const size_t n4 = ((size_t)S * S + 3) / 4 * 4;
  if (3 * n4 <= (size_t)kColorLdsBytes)
    hipLaunchKernelGGL(color_kernel<true>, dim3((unsigned)B), dim3(kColorThreads), 0, st, S, (uint8_t*)pix,
                       (const int*)prog_dev, desc, mean, stdv, out_uint8, out);
  else
    hipLaunchKernelGGL(color_kernel<false>, dim3((unsigned)B), dim3(kColorThreads), 0, st, S, (uint8_t*)pix,
                       (const int*)prog_dev, desc, mean, stdv, out_uint8, out);
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

extern "C" int clipk_image_color(int B, int S, void* pix, const int* prog, int* prog_dev, const float* mean,
                                 const float* stdv, int out_uint8, void* out, void* stream) {
  return color_launch(B, S, CLIPK_COLOR_DESC, pix, prog, prog_dev, mean, stdv, out_uint8, out, stream);
}

extern "C" int clipk_image_color_blur(int B, int S, void* pix, const int* prog, int* prog_dev, const float* mean,
                                      const float* stdv, int out_uint8, void* out, void* stream) {
  return color_launch(B, S, CLIPK_COLORBLUR_DESC, pix, prog, prog_dev, mean, stdv, out_uint8, out, stream);
}
