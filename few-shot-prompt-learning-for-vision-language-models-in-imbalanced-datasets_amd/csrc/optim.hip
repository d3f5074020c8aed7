// Multi-tensor Adam / AdamW / AMSGrad step (torch.optim.Adam / AdamW, the non-capturable
// single-tensor form; Dassl optim/optimizer.py builds them for OPTIM.NAME adam / amsgrad / adamw).
// The launch shape of sgd_multi_kernel (prompt.hip): up to 16 tensors of a param group per launch,
// tensor blockIdx.y, grid-stride over its elements, 256 threads per block.
//
// Memory-bound: per element 16 B read (p, g, m, v) + 12 B written (p, m, v); AMSGrad 20 + 16. A
// tensor whose pointers are all 16-byte aligned moves 16 B per lane and access (its last n % 4
// elements one by one); any other tensor -- a contiguous view at a 4-byte offset -- one element
// per lane.
//
// The step count t lives on the device, per tensor (torch keeps `step` per parameter), because a
// guarded launch (guard[0] & mask, the PREC fp32s overflow flag) must leave it where it was
// without the host knowing: two int32 counters step[k][0..1]. A launch reads step[k][parity[k]]
// in every block and thread 0 of the tensor's block 0 writes step[k][parity[k] ^ 1] (t + 1, or t
// unchanged when the launch is skipped): no block reads the word another one writes, launches on
// a stream are ordered, and the host flips a tensor's parity with every launch that names it.
#include "common.h"

namespace {

constexpr int kAdamMaxTensors = 16;
// grid-stride cap: 2048 blocks x 4 waves fill the 256 CUs' 32 wave slots each; one grid pass is
// 2048 * 256 accesses (x 4 elements for an aligned tensor)
constexpr int kAdamGridCap = 2048;

struct AdamTensors {
  float* p[kAdamMaxTensors];
  const float* g[kAdamMaxTensors];
  float* m[kAdamMaxTensors];
  float* v[kAdamMaxTensors];
  float* vmax[kAdamMaxTensors];
  int* step[kAdamMaxTensors];
  long n[kAdamMaxTensors];
  int parity[kAdamMaxTensors];
};

struct AdamConsts {
  float b1, omb1, b2, omb2;  // beta, 1 - beta (formed in double on the host)
  float eps;
  float wd;                  // Adam / AMSGrad: weight_decay; AdamW: 1 - lr * weight_decay
  float gs;                  // gradient scale (SCALED)
  float step_size;           // lr / (1 - beta1^t)
  float bc2_sqrt;            // sqrt(1 - beta2^t)
};

__device__ __forceinline__ double pow_int(double b, int e) {
  double r = 1.0;
  for (; e > 0; e >>= 1, b *= b)
    if (e & 1) r *= b;
  return r;
}

// Every product and sum spelled out (no contraction left to the compiler): the SCALED and the
// plain instantiation then round alike, so a power-of-two scale is bitwise the update on
// pre-scaled gradients.
template <int MODE, bool SCALED>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vmax, const AdamConsts& c) {
  if (SCALED) g = __fmul_rn(g, c.gs);  // rounded on its own
  if (MODE == CLIPK_ADAM_ADAMW)
    p = __fmul_rn(p, c.wd);
  else
    g = __builtin_fmaf(c.wd, p, g);
  m = __builtin_fmaf(c.b1, m, __fmul_rn(c.omb1, g));
  v = __builtin_fmaf(c.b2, v, __fmul_rn(c.omb2, __fmul_rn(g, g)));
  float d = v;
  if (MODE == CLIPK_ADAM_AMSGRAD) {
    vmax = (v > vmax || v != v) ? v : vmax;  // torch.maximum: a NaN propagates
    d = vmax;
  }
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(d), c.bc2_sqrt), c.eps);
  p = __builtin_fmaf(-c.step_size, __fdiv_rn(m, denom), p);
}

template <int MODE, bool SCALED>
__global__ __launch_bounds__(256) void adam_multi_kernel(AdamTensors t, double lr, double beta1, double beta2,
                                                         AdamConsts c, const int* __restrict__ guard, int mask) {
  const int k = blockIdx.y;
  int* const st = t.step[k];
  const int par = t.parity[k];
  const int t0 = st[par];
  const bool skip = guard && (guard[0] & mask);
  if (blockIdx.x == 0 && threadIdx.x == 0) st[par ^ 1] = skip ? t0 : t0 + 1;
  if (skip) return;
  // 1 - beta^t in double (fp32 loses ~4 digits of 1 - 0.999^1), the step size rounded to fp32
  // as torch hands it to addcdiv_
  c.step_size = (float)(lr / (1.0 - pow_int(beta1, t0 + 1)));
  c.bc2_sqrt = (float)sqrt(1.0 - pow_int(beta2, t0 + 1));

  const long n = t.n[k];
  float* __restrict__ p = t.p[k];
  const float* __restrict__ g = t.g[k];
  float* __restrict__ m = t.m[k];
  float* __restrict__ v = t.v[k];
  float* __restrict__ vx = MODE == CLIPK_ADAM_AMSGRAD ? t.vmax[k] : nullptr;
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vx;
  long first = 0;  // where the one-by-one elements start
  if ((bits & 15) == 0) {
    const long nv = n >> 2;
    for (long i = tid; i < nv; i += stride) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
      f32x4 xx = {0.f, 0.f, 0.f, 0.f};
      if (MODE == CLIPK_ADAM_AMSGRAD) xx = reinterpret_cast<f32x4*>(vx)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pp[j], mj = mm[j], vj = vv[j], xj = xx[j];
        adam_elem<MODE, SCALED>(pj, gg[j], mj, vj, xj, c);
        pp[j] = pj; mm[j] = mj; vv[j] = vj; xx[j] = xj;
      }
      reinterpret_cast<f32x4*>(p)[i] = pp;
      reinterpret_cast<f32x4*>(m)[i] = mm;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      if (MODE == CLIPK_ADAM_AMSGRAD) reinterpret_cast<f32x4*>(vx)[i] = xx;
    }
    first = nv << 2;
  }
  for (long i = first + tid; i < n; i += stride) {
    float pj = p[i], mj = m[i], vj = v[i], xj = MODE == CLIPK_ADAM_AMSGRAD ? vx[i] : 0.f;
    adam_elem<MODE, SCALED>(pj, g[i], mj, vj, xj, c);
    p[i] = pj; m[i] = mj; v[i] = vj;
    if (MODE == CLIPK_ADAM_AMSGRAD) vx[i] = xj;
  }
}

template <int MODE>
void launch(dim3 grid, hipStream_t st, const AdamTensors& t, double lr, double beta1, double beta2,
            const AdamConsts& c, const int* guard, int mask) {
  if (c.gs == 1.0f)
    hipLaunchKernelGGL((adam_multi_kernel<MODE, false>), grid, dim3(256), 0, st, t, lr, beta1, beta2, c, guard, mask);
  else
    hipLaunchKernelGGL((adam_multi_kernel<MODE, true>), grid, dim3(256), 0, st, t, lr, beta1, beta2, c, guard, mask);
}

}  // namespace

extern "C" int clipk_adam_step_multi(int count, float* const* p, const float* const* g, float* const* m,
                                     float* const* v, float* const* vmax, const long* n, int* const* step,
                                     const int* parity, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, int mode, float grad_scale, const int* guard, int mask,
                                     void* stream) {
  if (count < 1 || count > kAdamMaxTensors || !p || !g || !m || !v || !n || !step || !parity) return CLIPK_EINVAL;
  if (mode != CLIPK_ADAM_ADAM && mode != CLIPK_ADAM_ADAMW && mode != CLIPK_ADAM_AMSGRAD) return CLIPK_EINVAL;
  if (mode == CLIPK_ADAM_AMSGRAD && !vmax) return CLIPK_EINVAL;
  // (written so that a NaN fails too)
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(lr >= 0.0) ||
      !(weight_decay >= 0.0))
    return CLIPK_EINVAL;
  AdamTensors t{};
  long work = 0;  // accesses of the longest tensor: 4 elements each when it is 16-byte aligned
  for (int k = 0; k < count; ++k) {
    if (!p[k] || !g[k] || !m[k] || !v[k] || !step[k] || (mode == CLIPK_ADAM_AMSGRAD && !vmax[k])) return CLIPK_EINVAL;
    if (parity[k] != 0 && parity[k] != 1) return CLIPK_EINVAL;
    if (n[k] < 0) return CLIPK_ESHAPE;
    t.p[k] = p[k];
    t.g[k] = g[k];
    t.m[k] = m[k];
    t.v[k] = v[k];
    t.vmax[k] = mode == CLIPK_ADAM_AMSGRAD ? vmax[k] : nullptr;
    t.step[k] = step[k];
    t.n[k] = n[k];
    t.parity[k] = parity[k];
    const uintptr_t bits = (uintptr_t)t.p[k] | (uintptr_t)t.g[k] | (uintptr_t)t.m[k] | (uintptr_t)t.v[k] |
                           (uintptr_t)t.vmax[k];
    const long w = (bits & 15) ? n[k] : (n[k] + 3) >> 2;
    work = w > work ? w : work;
  }
  AdamConsts c{};
  c.b1 = (float)beta1;
  c.omb1 = (float)(1.0 - beta1);
  c.b2 = (float)beta2;
  c.omb2 = (float)(1.0 - beta2);
  c.eps = (float)eps;
  c.wd = mode == CLIPK_ADAM_ADAMW ? (float)(1.0 - lr * weight_decay) : (float)weight_decay;
  c.gs = grad_scale;
  // (a launch even when every tensor is empty: the step counts advance as torch's do)
  long blocks = (work + 255) / 256;
  blocks = blocks > kAdamGridCap ? kAdamGridCap : (blocks < 1 ? 1 : blocks);
  const dim3 grid((unsigned)blocks, (unsigned)count);
  const hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case CLIPK_ADAM_ADAM: launch<CLIPK_ADAM_ADAM>(grid, st, t, lr, beta1, beta2, c, guard, mask); break;
    case CLIPK_ADAM_ADAMW: launch<CLIPK_ADAM_ADAMW>(grid, st, t, lr, beta1, beta2, c, guard, mask); break;
    default: launch<CLIPK_ADAM_AMSGRAD>(grid, st, t, lr, beta1, beta2, c, guard, mask); break;
  }
  CLIPK_CHECK_LAUNCH();
  return CLIPK_OK;
}
