// Convolution kernels of CLIP's ModifiedResNet (PromptSRC/clip/model.py:10-150), frozen and
// forward-only: an NHWC implicit-GEMM convolution on the gfx950 MFMA with the frozen BatchNorm,
// the residual add and the ReLU in its epilogue, the stem's 3x3 / stride-2 gather, the 2x2 average
// pool and the single-query attention of AttentionPool2d. No atomics, no split-K: every output
// element is one wave's fixed-order sum, so two calls agree bitwise.
#include <algorithm>

#include "common.h"

namespace clipk {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- conv2d (implicit GEMM)
// out[m, n] = epi( sum_k A[m, k] W[n, k] ),  m = (b, oy, ox),  k = (tap, c) tap-major, c fastest.
// A K step is 32 elements; Cin % 32 == 0 keeps a step inside one tap, so each lane's slice of A is
// one 16-B load from x (two for fp32) and the tap's offset is uniform over the block.
//   16-bit: mfma_f32_16x16x32: lane l supplies row / col l & 15 and k = 8 (l >> 4) .. + 7.
//   fp32:   mfma_f32_16x16x4f32, 8 per step: MFMA (h, i) takes k = 16 h + 4 (l >> 4) + i from the
//           lane's two 16-B chunks -- the same permutation of k on A and on W, so the sum is over
//           every k once.
// Block = 4 waves = 64 FR rows x BN columns; a wave owns 16 FR rows (FR = 1 or 2 A fragments, loaded
// straight from x) x BN columns (BN / 16 W fragments from the LDS tile the block shares, double
// buffered: one barrier per K step).
// Halo: a tap outside the image, or a row m >= M, selects zero AFTER a load whose index was clamped
// into the same image ([0, H) x [0, W); rows m >= M take pixel M - 1), so no address outside x is
// ever formed.
template <typename T>
__device__ __forceinline__ f32x4 conv_mfma(const i32x4* a, const i32x4* b, f32x4 c) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 fa = __builtin_bit_cast(f32x4, a[h]), fb = __builtin_bit_cast(f32x4, b[h]);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0], fb[0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1], fb[1], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[2], fb[2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[3], fb[3], c, 0, 0, 0);
    }
    return c;
  } else if constexpr (__is_same(T, f16)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[0]), c,
                                                  0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[0]), __builtin_bit_cast(bf16x8, b[0]),
                                                   c, 0, 0, 0);
  }
}

template <typename T, int BN, int FR, bool OUT32>
__global__ __launch_bounds__(256) void conv_kernel(long M, int H, int W, int Cin, int Cout, int ksize, int flags,
                                                   const T* __restrict__ x, const T* __restrict__ w,
                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                   const T* __restrict__ res, void* __restrict__ out) {
  constexpr int BK = 32, NJ = BN / 16, EPC = 16 / (int)sizeof(T), NCH = sizeof(T) == 4 ? 2 : 1;
  constexpr int ROWB = BK * (int)sizeof(T) + 16;  // LDS row stride (bytes): + 16 B spreads the banks
  constexpr int CPR = BK * (int)sizeof(T) / 16, NB = BN * CPR, NBL = (NB + 255) / 256;
  __shared__ CLIPK_LDS_ALIGN char lds[2][BN * ROWB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
  const long m0 = (long)blockIdx.x * (64 * FR) + wave * (16 * FR);
  const int n0 = blockIdx.y * BN;
  const int K = ksize * ksize * Cin;
  const int HW = H * W;

  int py[FR], px[FR];
  long pimg[FR];
  bool pv[FR];
#pragma unroll
  for (int f = 0; f < FR; ++f) {
    const long m = m0 + f * 16 + r;
    pv[f] = m < M;
    const long mc = pv[f] ? m : M - 1;
    const int pix = (int)(mc % HW);
    pimg[f] = mc - pix;  // first pixel of the row's image
    py[f] = pix / W;
    px[f] = pix % W;
  }

  i32x4 a_cur[FR][NCH], a_nxt[FR][NCH], breg[NBL];
  auto load_a = [&](int k0, i32x4 (*a)[NCH]) {
    const int tap = k0 / Cin, c0 = k0 - tap * Cin;
    const int dy = ksize == 3 ? tap / 3 - 1 : 0, dx = ksize == 3 ? tap % 3 - 1 : 0;
#pragma unroll
    for (int f = 0; f < FR; ++f) {
      const int iy = py[f] + dy, ix = px[f] + dx;
      const bool inb = pv[f] && iy >= 0 && iy < H && ix >= 0 && ix < W;
      const int iyc = min(max(iy, 0), H - 1), ixc = min(max(ix, 0), W - 1);
      const T* p = x + (size_t)(pimg[f] + iyc * W + ixc) * Cin + c0 + g * EPC;
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        const i32x4 v = *reinterpret_cast<const i32x4*>(p + h * 16);
        a[f][h] = inb ? v : i32x4{0, 0, 0, 0};
      }
    }
  };
  auto load_b = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int idx = tid + i * 256;
      if (idx < NB)
        breg[i] = *reinterpret_cast<const i32x4*>(w + (size_t)(n0 + idx / CPR) * K + k0 + (idx % CPR) * EPC);
    }
  };
  auto store_b = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int idx = tid + i * 256;
      if (idx < NB) *reinterpret_cast<i32x4*>(&lds[buf][(idx / CPR) * ROWB + (idx % CPR) * 16]) = breg[i];
    }
  };

  f32x4 acc[FR][NJ];
#pragma unroll
  for (int f = 0; f < FR; ++f)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_a(0, a_cur);
  load_b(0);
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    // the readers of lds[buf] (two steps ago) passed the previous step's barrier before this write
    store_b(buf);
    __syncthreads();
    const bool more = k0 + BK < K;
    if (more) {
      load_a(k0 + BK, a_nxt);
      load_b(k0 + BK);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      i32x4 b[NCH];
#pragma unroll
      for (int h = 0; h < NCH; ++h)
        b[h] = *reinterpret_cast<const i32x4*>(&lds[buf][(j * 16 + r) * ROWB + h * 64 + g * 16]);
#pragma unroll
      for (int f = 0; f < FR; ++f) acc[f][j] = conv_mfma<T>(a_cur[f], b, acc[f][j]);
    }
    if (more) {
#pragma unroll
      for (int f = 0; f < FR; ++f)
#pragma unroll
        for (int h = 0; h < NCH; ++h) a_cur[f][h] = a_nxt[f][h];
    }
    buf ^= 1;
  }

  // epilogue: C/D map col = lane & 15, row = 4 (lane >> 4) + i
  const bool has_res = flags & CLIPK_CONV_RES, relu = flags & CLIPK_CONV_RELU;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = n0 + j * 16 + r;
    const float sc = scale ? scale[n] : 1.f, sh = shift ? shift[n] : 0.f;
#pragma unroll
    for (int f = 0; f < FR; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long m = m0 + f * 16 + 4 * g + i;
        if (m < M) {
          const size_t o = (size_t)m * Cout + n;
          float v = fmaf(acc[f][j][i], sc, sh);
          if (has_res) v += to_f32(res[o]);
          if (relu) v = fmaxf(v, 0.f);
          if constexpr (OUT32) reinterpret_cast<float*>(out)[o] = v;
          else reinterpret_cast<T*>(out)[o] = from_f32<T>(v);
        }
      }
  }
}

// Tile choice: 128 rows x 64 columns per block while that fills the 256 CUs at least twice, else 128 x 32,
// else 64 x 32 (the 14x14 and 7x7 maps at small batches). Every choice sums an output's products in the
// same order, so the result does not depend on it.
template <typename T>
static int conv_launch(int flags, long M, int H, int W, int Cin, int Cout, int ksize, const void* x, const void* w,
                       const float* scale, const float* shift, const void* res, void* out, hipStream_t st) {
  const bool o32 = (flags & CLIPK_CONV_OUT_F32) && sizeof(T) != 4;
  constexpr long kFill = 2 * 256;
  int bn = 32, fr = 1;
  if (Cout % 64 == 0 && ((M + 127) / 128) * (Cout / 64) >= kFill) bn = 64, fr = 2;
  else if (((M + 127) / 128) * (Cout / 32) >= kFill) fr = 2;
  const dim3 grid((unsigned)((M + 64 * fr - 1) / (64 * fr)), Cout / bn);
#define CONV_GO(BN, FR, O32)                                                                                   \
  hipLaunchKernelGGL((conv_kernel<T, BN, FR, O32>), grid, 256, 0, st, M, H, W, Cin, Cout, ksize, flags, (const T*)x, \
                     (const T*)w, scale, shift, (const T*)res, out)
  if (bn == 64) {
    if (o32) CONV_GO(64, 2, true); else CONV_GO(64, 2, false);
  } else if (fr == 2) {
    if (o32) CONV_GO(32, 2, true); else CONV_GO(32, 2, false);
  } else {
    if (o32) CONV_GO(32, 1, true); else CONV_GO(32, 1, false);
  }
#undef CONV_GO
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

// ---------------------------------------------------------------- stem gather (conv1: 3x3, stride 2, pad 1)
// img fp32 [B,3,R,R] -> out [B (R/2)^2, 32]: k = (ky*3 + kx)*3 + c for k < 27, zero for 27..31.
// Taps outside the image: index clamped, zero selected.
template <typename TO>
__global__ __launch_bounds__(256) void im2col_3x3s2_kernel(int B, int R, const float* __restrict__ img,
                                                           TO* __restrict__ out) {
  const int Ho = R / 2;
  const long total = (long)B * Ho * Ho * 32;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int k = (int)(e & 31);
    const long pix = e >> 5;
    float v = 0.f;
    if (k < 27) {
      const int b = (int)(pix / (Ho * Ho)), pi = (int)(pix % (Ho * Ho));
      const int oy = pi / Ho, ox = pi % Ho;
      const int tap = k / 3, c = k % 3;
      const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
      const bool inb = iy >= 0 && iy < R && ix >= 0 && ix < R;
      const int iyc = min(max(iy, 0), R - 1), ixc = min(max(ix, 0), R - 1);
      const float t = img[(((long)b * 3 + c) * R + iyc) * R + ixc];
      v = inb ? t : 0.f;
    }
    out[e] = (TO)v;
  }
}

// ---------------------------------------------------------------- 2x2 average pool, stride 2 (NHWC)
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_kernel(int B, int H, int W, int C, const T* __restrict__ x,
                                                       T* __restrict__ out) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int Ho = H / 2, Wo = W / 2, CC = C / EPC;
  const long total = (long)B * Ho * Wo * CC;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int cc = (int)(e % CC);
    long p = e / CC;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const long b = p / Ho;
    const T* s = x + ((size_t)(b * H + 2 * oy) * W + 2 * ox) * C + cc * EPC;
    float v0[EPC], v1[EPC], v2[EPC], v3[EPC], o[EPC];
    load16_f32(s, v0);
    load16_f32(s + C, v1);
    load16_f32(s + (size_t)W * C, v2);
    load16_f32(s + (size_t)W * C + C, v3);
#pragma unroll
    for (int i = 0; i < EPC; ++i) o[i] = ((v0[i] + v1[i]) + (v2[i] + v3[i])) * 0.25f;
    store16_f32(out + (size_t)e * EPC, o);
  }
}

// ---------------------------------------------------------------- AttentionPool2d (model.py:58-91)
// tokens: tok[b, 0] = mean_i x[b, i] + pos[0] (fp32 sum in pixel order), tok[b, 1 + i] = x[b, i] +
// pos[1 + i], rounded once to T; qin[b] = tok[b, 0], the only query row.
template <typename T>
__global__ __launch_bounds__(256) void attnpool_tokens_kernel(int HW, int C, const T* __restrict__ x,
                                                              const float* __restrict__ pos, T* __restrict__ tok,
                                                              T* __restrict__ qin) {
  const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const T* xb = x + (size_t)b * HW * C;
  T* tb = tok + (size_t)b * (HW + 1) * C;
  float sum = 0.f;
  for (int i = 0; i < HW; ++i) {
    const float v = to_f32(xb[(size_t)i * C + c]);
    sum += v;
    tb[(size_t)(i + 1) * C + c] = from_f32<T>(v + pos[(size_t)(i + 1) * C + c]);
  }
  const T t0 = from_f32<T>(sum / (float)HW + pos[c]);
  tb[c] = t0;
  qin[(size_t)b * C + c] = t0;
}

// One wave per (image, head), head dim 64: scores of the single query against L <= 256 keys
// (lane j takes keys j, j + 64, ...), fp32 softmax, then lane d sums p_j v[j][d].
template <typename T>
__global__ __launch_bounds__(64) void attnpool_attn_kernel(int L, int C, int heads, const T* __restrict__ q,
                                                           const T* __restrict__ kv, T* __restrict__ o) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ float qs[64], ps[256];
  const int b = blockIdx.x / heads, h = blockIdx.x % heads, lane = threadIdx.x;
  qs[lane] = to_f32(q[(size_t)b * C + h * 64 + lane]) * 0.125f;  // 64^-0.5
  __syncthreads();
  float s[4], mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    s[t] = -INFINITY;
    if (j < L) {
      const T* kp = kv + (size_t)(b * L + j) * 2 * C + h * 64;
      float acc = 0.f;
      for (int d = 0; d < 64; d += EPC) {
        float v[EPC];
        load16_f32(kp + d, v);
#pragma unroll
        for (int i = 0; i < EPC; ++i) acc = fmaf(qs[d + i], v[i], acc);
      }
      s[t] = acc;
    }
    mx = fmaxf(mx, s[t]);
  }
  mx = wave_max(mx);
  float tot = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    const float e = j < L ? expf(s[t] - mx) : 0.f;
    ps[j] = e;
    tot += e;
  }
  tot = wave_sum(tot);
  __syncthreads();
  float acc = 0.f;
  const T* vp = kv + (size_t)b * L * 2 * C + C + h * 64 + lane;
  for (int j = 0; j < L; ++j) acc = fmaf(ps[j], to_f32(vp[(size_t)j * 2 * C]), acc);
  o[(size_t)b * C + h * 64 + lane] = from_f32<T>(acc / tot);
}

static inline int grid_1d(long total) { return (int)std::min<long>((total + 255) / 256, 1 << 20); }
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline size_t esz(int dt) { return dt == CLIPK_F32 ? 4 : 2; }
static inline size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace clipk

using namespace clipk;

extern "C" int clipk_conv2d_nhwc(int dtype, int flags, int B, int H, int W, int Cin, int Cout, int ksize,
                                 const void* x, const void* w, const float* scale, const float* shift,
                                 const void* res, void* out, void* stream) {
  if (!x || !w || !out || !al16(x) || !al16(w) || !al16(out)) return CLIPK_EINVAL;
  if (flags & ~(CLIPK_CONV_RES | CLIPK_CONV_RELU | CLIPK_CONV_OUT_F32)) return CLIPK_EINVAL;
  if ((flags & CLIPK_CONV_RES) && !res) return CLIPK_EINVAL;
  if (dtype != CLIPK_F32 && dtype != CLIPK_F16 && dtype != CLIPK_BF16) return CLIPK_EINVAL;
  if (ksize != 1 && ksize != 3) return CLIPK_EINVAL;
  if (B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 32 || Cout % 32) return CLIPK_EINVAL;
  if ((long)H * W > (1L << 24) || Cout / 32 > 65535) return CLIPK_EINVAL;
  const long M = (long)B * H * W;
  if (M == 0) return CLIPK_OK;
  if ((M + 63) / 64 > 0x7fffffffL) return CLIPK_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case CLIPK_F16: return conv_launch<f16>(flags, M, H, W, Cin, Cout, ksize, x, w, scale, shift, res, out, st);
    case CLIPK_BF16: return conv_launch<bf16>(flags, M, H, W, Cin, Cout, ksize, x, w, scale, shift, res, out, st);
    default: return conv_launch<float>(flags, M, H, W, Cin, Cout, ksize, x, w, scale, shift, res, out, st);
  }
}

extern "C" int clipk_im2col_3x3s2(int out_dtype, int B, int res, const float* img, void* out, void* stream) {
  if (!img || !out || B < 0 || res <= 0 || res % 2) return CLIPK_EINVAL;
  const long total = (long)B * (res / 2) * (res / 2) * 32;
  if (total == 0) return CLIPK_OK;
  hipStream_t st = (hipStream_t)stream;
  const int grid = grid_1d(total);
  switch (out_dtype) {
    case CLIPK_F16: hipLaunchKernelGGL(im2col_3x3s2_kernel<f16>, grid, 256, 0, st, B, res, img, (f16*)out); break;
    case CLIPK_BF16: hipLaunchKernelGGL(im2col_3x3s2_kernel<bf16>, grid, 256, 0, st, B, res, img, (bf16*)out); break;
    case CLIPK_F32: hipLaunchKernelGGL(im2col_3x3s2_kernel<float>, grid, 256, 0, st, B, res, img, (float*)out); break;
    default: return CLIPK_EINVAL;
  }
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

extern "C" int clipk_avgpool2_nhwc(int dtype, int B, int H, int W, int C, const void* x, void* out, void* stream) {
  if (!x || !out || !al16(x) || !al16(out)) return CLIPK_EINVAL;
  if (B < 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || C <= 0 || C % 8) return CLIPK_EINVAL;
  const long total = (long)B * (H / 2) * (W / 2) * (C / (16 / (int)esz(dtype)));
  if (total == 0) return CLIPK_OK;
  hipStream_t st = (hipStream_t)stream;
  const int grid = grid_1d(total);
  switch (dtype) {
    case CLIPK_F16: hipLaunchKernelGGL(avgpool2_kernel<f16>, grid, 256, 0, st, B, H, W, C, (const f16*)x, (f16*)out); break;
    case CLIPK_BF16: hipLaunchKernelGGL(avgpool2_kernel<bf16>, grid, 256, 0, st, B, H, W, C, (const bf16*)x, (bf16*)out); break;
    case CLIPK_F32: hipLaunchKernelGGL(avgpool2_kernel<float>, grid, 256, 0, st, B, H, W, C, (const float*)x, (float*)out); break;
    default: return CLIPK_EINVAL;
  }
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}

extern "C" size_t clipk_attnpool_ws_bytes(int dtype, int B, int HW, int C) {
  const size_t e = esz(dtype), L = (size_t)HW + 1, b = (size_t)std::max(B, 0);
  // tok [B L, C], kv [B L, 2C], qin / q / o [B, C]
  return up256(b * L * C * e) + up256(b * L * 2 * C * e) + 3 * up256(b * C * e);
}

extern "C" int clipk_attnpool(int dtype, int B, int HW, int C, int heads, int E, const void* x, const float* pos,
                              const void* q_w, const float* q_b, const void* kv_w, const float* kv_b,
                              const void* c_w, const float* c_b, float* feat, void* ws, size_t ws_bytes,
                              void* stream) {
  if (!x || !pos || !q_w || !q_b || !kv_w || !kv_b || !c_w || !c_b || !feat || !ws || !al16(ws)) return CLIPK_EINVAL;
  if (dtype != CLIPK_F32 && dtype != CLIPK_F16 && dtype != CLIPK_BF16) return CLIPK_EINVAL;
  if (B < 0 || HW <= 0 || HW + 1 > 256 || heads <= 0 || C != heads * 64 || E <= 0 || E % 32) return CLIPK_EINVAL;
  if (ws_bytes < clipk_attnpool_ws_bytes(dtype, B, HW, C)) return CLIPK_EWORKSPACE;
  if (B == 0) return CLIPK_OK;
  const size_t e = esz(dtype), L = (size_t)HW + 1;
  char* p = (char*)ws;
  void* tok = p; p += up256((size_t)B * L * C * e);
  void* kv = p; p += up256((size_t)B * L * 2 * C * e);
  void* qin = p; p += up256((size_t)B * C * e);
  void* q = p; p += up256((size_t)B * C * e);
  void* o = p;
  hipStream_t st = (hipStream_t)stream;
  const dim3 tg(B, (C + 255) / 256);
  switch (dtype) {
    case CLIPK_F16: hipLaunchKernelGGL(attnpool_tokens_kernel<f16>, tg, 256, 0, st, HW, C, (const f16*)x, pos, (f16*)tok, (f16*)qin); break;
    case CLIPK_BF16: hipLaunchKernelGGL(attnpool_tokens_kernel<bf16>, tg, 256, 0, st, HW, C, (const bf16*)x, pos, (bf16*)tok, (bf16*)qin); break;
    default: hipLaunchKernelGGL(attnpool_tokens_kernel<float>, tg, 256, 0, st, HW, C, (const float*)x, pos, (float*)tok, (float*)qin); break;
  }
  CLIPK_CHECK_LAUNCH();
  // projections as 1x1 convolutions (scale 1, shift = bias): k | v over every token, q on the mean rows
  int rc = clipk_conv2d_nhwc(dtype, 0, 1, 1, (int)(B * L), C, 2 * C, 1, tok, kv_w, nullptr, kv_b, nullptr, kv, stream);
  if (rc) return rc;
  rc = clipk_conv2d_nhwc(dtype, 0, 1, 1, B, C, C, 1, qin, q_w, nullptr, q_b, nullptr, q, stream);
  if (rc) return rc;
  switch (dtype) {
    case CLIPK_F16: hipLaunchKernelGGL(attnpool_attn_kernel<f16>, B * heads, 64, 0, st, (int)L, C, heads, (const f16*)q, (const f16*)kv, (f16*)o); break;
    case CLIPK_BF16: hipLaunchKernelGGL(attnpool_attn_kernel<bf16>, B * heads, 64, 0, st, (int)L, C, heads, (const bf16*)q, (const bf16*)kv, (bf16*)o); break;
    default: hipLaunchKernelGGL(attnpool_attn_kernel<float>, B * heads, 64, 0, st, (int)L, C, heads, (const float*)q, (const float*)kv, (float*)o); break;
  }
  CLIPK_CHECK_LAUNCH();
  return clipk_conv2d_nhwc(dtype, CLIPK_CONV_OUT_F32, 1, 1, B, C, E, 1, o, c_w, nullptr, c_b, nullptr, feat, stream);
}
