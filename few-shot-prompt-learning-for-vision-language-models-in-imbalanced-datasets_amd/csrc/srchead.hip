// PromptSRC head (clipk_src_head, include/clipk.h): the whole objective of
// PromptSRC.forward_backward (promptsrc.py:171-213, 296-323) and its gradients with respect to the
// raw prompted image / text features, from one call.
//
//   n(x) = x / max(|x|, 1e-12)   u_b = n(img_b)   t_c = n(txt_c)   z_b = n(zs_b)
//   s = scale u t^T   q = scale z fixed_q^T   ls, lq = row log-softmax of s, q
//   ce = mean_b L(s_b, y_b) (CE or focal, clipk_ce_loss's arithmetic)
//   kl = w_logits / (B C) sum exp(lq) (lq - ls)
//   l1_text = w_text / (C E) sum |t - fixed_n|      l1_image = w_image / (B E) sum |u - z|
//   G = d total / d s = wgt_b / B (softmax(s) - onehot) + w_logits / (B C) (softmax(s) - softmax(q))
//   g_u = scale G t + w_image / (B E) sign(u - z)   g_t = scale G^T u + w_text / (C E) sign(t - fixed_n)
//   d x = grad_scale (g - (g . n) n) / |x|
//
// Four launches, data handed on at kernel boundaries only:
//  1. dots_kernel   the raw products img txt^T and zs fixed_q^T (fp32 FMA chains) on 32 x 32 tiles, E
//                   cut into slices so that a small B x C still fills the device (slice partials to the
//                   workspace); further blocks of the same launch take one wave per row for 1 / |x| of
//                   img, zs, txt and the two L1 row sums.
//  2. rows_kernel   one block per image row: the slices summed in slice order and scaled to s and q,
//                   both log-sum-exps as the pair (row max, log of the sum), the CE / focal row loss,
//                   the KL row sum and G.
//  3. grad_kernel   one wave per text row: g_t, its projection and d_txt. Further waves of the same
//                   launch: the product G t for one image row and one slice of C (the d_img rows each
//                   walk all of txt: B waves alone would leave the device idle).
//  4. image_kernel  one wave per image row: the slices summed in slice order, the sign term, the
//                   projection and d_img; a last block sums the row losses into loss[0..4].
// Forward only: 1, 2 and loss_kernel. No atomics, every sum in a fixed order: bitwise reproducible.
// Global loads are unconditional on clamped (always in-bounds) indices, with a select for what lies
// outside (ntxent.hip has the reason).
#include "common.h"

using namespace clipk;

namespace {

constexpr int KC = 32;      // reduction-dimension elements per LDS stage
constexpr int RS = KC + 4;  // LDS row stride in floats
constexpr int T = 32;       // output tile edge: 256 threads x (2 x 2)
constexpr int MT = 2;
constexpr int kMaxB = 128;
constexpr int RU = 4;       // rows in flight of the gradient products

struct Plan {
  int tb, tc;    // tiles over B and C
  int splits;    // E slices of the two products
  int kchunk;    // E elements per slice (multiple of KC)
  int nprod;     // product blocks of dots_kernel
  int cslices;   // C slices of the d_img product
  int cchunk;    // classes per slice
};

Plan make_plan(int B, int C, int E) {
  Plan p;
  p.tb = (B + T - 1) / T;
  p.tc = (C + T - 1) / T;
  const long tiles = 2L * p.tb * p.tc;
  const int chunks = (E + KC - 1) / KC;
  long want = 256 / tiles;
  if (want < 1) want = 1;
  if (want > 16) want = 16;
  const int splits = want < chunks ? (int)want : chunks;
  p.kchunk = ((chunks + splits - 1) / splits) * KC;
  p.splits = (E + p.kchunk - 1) / p.kchunk;
  p.nprod = (int)(tiles * p.splits);
  int cs = 256 / B;  // ~256 waves over the B rows
  if (cs < 1) cs = 1;
  if (cs > 32) cs = 32;  // image_kernel walks the slices of its row one after the other
  const int cmax = (C + 15) / 16;  // at least 16 classes per slice
  if (cs > cmax) cs = cmax;
  p.cchunk = (C + cs - 1) / cs;
  p.cslices = (C + p.cchunk - 1) / p.cchunk;
  return p;
}

struct Ws {
  float *ri_img, *ri_zs, *ri_txt, *l1i, *l1t, *rowce, *rowkl, *part, *S, *Q, *G, *dpart;
  size_t floats;
};

// base may be null (clipk_src_head_ws_bytes): only floats is meaningful then
Ws carve(float* base, int B, int C, int E, const Plan& p) {
  Ws w;
  const size_t bc = (size_t)B * C;
  size_t o = 0;
  auto take = [&](size_t n) {
    float* f = base ? base + o : nullptr;
    o += n;
    return f;
  };
  w.ri_img = take(B);
  w.ri_zs = take(B);
  w.ri_txt = take(C);
  w.l1i = take(B);
  w.l1t = take(C);
  w.rowce = take(B);
  w.rowkl = take(B);
  w.part = take(2 * (size_t)p.splits * bc);
  w.S = take(bc);
  w.Q = take(bc);
  w.G = take(bc);
  w.dpart = take((size_t)p.cslices * B * E);
  w.floats = o;
  return w;
}

__device__ __forceinline__ float sign0(float d) { return (d > 0.f ? 1.f : 0.f) - (d < 0.f ? 1.f : 0.f); }

// One wave: ra = 1 / max(|a|, 1e-12), rb likewise (or 1 when b is already normalised), and
// sum_e |a ra - b rb| -- the same expressions the gradient kernels take the sign of.
__device__ __forceinline__ void norm_row(int E, int lane, const float* __restrict__ a, const float* __restrict__ b,
                                         bool norm_b, float& ra, float& rb, float& l1) {
  float sa = 0.f, sb = 0.f;
  for (int e0 = 0; e0 < E; e0 += 64) {
    const int e = e0 + lane, ec = min(e, E - 1);
    const float va = a[ec], vb = b[ec];
    const bool ok = e < E;
    sa = fmaf(ok ? va : 0.f, va, sa);
    sb = fmaf(ok ? vb : 0.f, vb, sb);
  }
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  ra = 1.0f / fmaxf(sqrtf(sa), 1e-12f);  // F.normalize's clamp
  rb = norm_b ? 1.0f / fmaxf(sqrtf(sb), 1e-12f) : 1.0f;
  float s = 0.f;
  for (int e0 = 0; e0 < E; e0 += 64) {
    const int e = e0 + lane, ec = min(e, E - 1);
    const float va = a[ec], vb = b[ec];
    s += e < E ? fabsf(va * ra - vb * rb) : 0.f;
  }
  l1 = wave_sum(s);
}

// Blocks [0, nprod): part[z][slice][b][c] = sum_{k in slice} A_b[k] M_c[k], (A, M) = (img, txt) for
// z = 0 and (zs, fixed_q) for z = 1; thread (tx, ty) owns rows ty + 16 m and columns tx + 16 c of the
// tile (gram_kernel of ntxent.hip). Blocks after them: one wave per row of norm_row.
__global__ __launch_bounds__(256) void dots_kernel(int B, int C, int E, int tb, int tc, int splits, int kchunk,
                                                   int nprod, const float* __restrict__ img,
                                                   const float* __restrict__ txt, const float* __restrict__ zs,
                                                   const float* __restrict__ fixed_n,
                                                   const float* __restrict__ fixed_q, float* __restrict__ part,
                                                   float* __restrict__ ri_img, float* __restrict__ ri_zs,
                                                   float* __restrict__ ri_txt, float* __restrict__ l1i,
                                                   float* __restrict__ l1t) {
  const int t = threadIdx.x;
  if ((int)blockIdx.x >= nprod) {
    const int lane = t & 63;
    const long w = ((long)blockIdx.x - nprod) * 4 + (t >> 6);
    float ra, rb, l1;
    if (w < B) {
      norm_row(E, lane, img + (size_t)w * E, zs + (size_t)w * E, true, ra, rb, l1);
      if (lane == 0) {
        ri_img[w] = ra;
        ri_zs[w] = rb;
        l1i[w] = l1;
      }
    } else if (w - B < C) {
      const long c = w - B;
      norm_row(E, lane, txt + (size_t)c * E, fixed_n + (size_t)c * E, false, ra, rb, l1);
      if (lane == 0) {
        ri_txt[c] = ra;
        l1t[c] = l1;
      }
    }
    return;
  }
  constexpr int P = T / 8;  // loader passes of 8 rows
  __shared__ CLIPK_LDS_ALIGN float As[T * RS];
  __shared__ CLIPK_LDS_ALIGN float Bs[T * RS];
  int idx = blockIdx.x;
  const int jt = idx % tc;
  idx /= tc;
  const int it = idx % tb;
  idx /= tb;
  const int sl = idx % splits;
  const int z = idx / splits;
  const float* A = z ? zs : img;
  const float* M = z ? fixed_q : txt;
  const int tx = t & 15, ty = t >> 4;
  const int lk = t & 31, lr = t >> 5;  // loader: k within the stage, row within a pass
  const int I0 = it * T, J0 = jt * T;
  const int k0 = sl * kchunk;
  const int k1 = min(E, k0 + kchunk);
  const float* pa[P];
  const float* pb[P];
  bool va[P], vb[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = I0 + p * 8 + lr, j = J0 + p * 8 + lr;
    va[p] = i < B;
    vb[p] = j < C;
    pa[p] = A + (size_t)min(i, B - 1) * E;
    pb[p] = M + (size_t)min(j, C - 1) * E;
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
  float* out = part + ((size_t)z * splits + sl) * B * C;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int i = I0 + ty + 16 * m;
#pragma unroll
    for (int c = 0; c < MT; ++c) {
      const int j = J0 + tx + 16 * c;
      if (i < B && j < C) out[(size_t)i * C + j] = acc[m][c];
    }
  }
}

// The four waves' values combined in wave order (fixed); every thread gets the result.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* sm) {
  v = MAX ? wave_max(v) : wave_sum(v);
  __syncthreads();  // sm free again
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])) : ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// Block b: thread t owns columns t, t + 256, ... in every pass, so the s and q it stores in the
// first pass are its own to read back in the later ones.
__global__ __launch_bounds__(256) void rows_kernel(int B, int C, int splits, float scale,
                                                   const float* __restrict__ part,
                                                   const float* __restrict__ ri_img, const float* __restrict__ ri_zs,
                                                   const float* __restrict__ ri_txt,
                                                   const int64_t* __restrict__ labels,
                                                   const float* __restrict__ alpha, float gamma, int focal,
                                                   float inv_b, float klw, float* S, float* Q,
                                                   float* __restrict__ G, float* __restrict__ rowce,
                                                   float* __restrict__ rowkl) {
  __shared__ float sm[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const size_t bc = (size_t)B * C;
  const size_t row = (size_t)b * C;
  const int64_t y = labels[b];
  const bool yok = y >= 0 && y < C;
  const float ru = ri_img[b], rz = ri_zs[b];
  float ms = -INFINITY, mq = -INFINITY, sy = 0.f;
  for (int c = t; c < C; c += 256) {
    float ds = 0.f, dq = 0.f;
    for (int k0 = 0; k0 < splits; k0 += RU) {  // RU slices in flight, added in slice order
      float vs[RU], vq[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int k = min(k0 + u, splits - 1);
        vs[u] = part[(size_t)k * bc + row + c];
        vq[u] = part[(size_t)(splits + k) * bc + row + c];
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        ds += k0 + u < splits ? vs[u] : 0.f;
        dq += k0 + u < splits ? vq[u] : 0.f;
      }
    }
    const float s = ds * (ru * ri_txt[c]) * scale;
    const float q = dq * rz * scale;
    S[row + c] = s;
    Q[row + c] = q;
    ms = fmaxf(ms, s);
    mq = fmaxf(mq, q);
    sy += (c == y) ? s : 0.f;  // one thread holds it, the others add zeros
  }
  ms = block_reduce<true>(ms, sm);
  mq = block_reduce<true>(mq, sm);
  sy = block_reduce<false>(sy, sm);
  float es = 0.f, eq = 0.f;
  for (int c = t; c < C; c += 256) {
    es += expf(S[row + c] - ms);
    eq += expf(Q[row + c] - mq);
  }
  const float lgs = logf(block_reduce<false>(es, sm));
  const float lgq = logf(block_reduce<false>(eq, sm));
  // clipk_ce_loss's row terms; a label outside [0, C) was never dereferenced: NaN
  float l, wgt;
  if (!yok) {
    l = wgt = __builtin_nanf("");
  } else {
    const float ce = (ms - sy) + lgs;
    l = ce;
    wgt = 1.f;
    if (focal) {
      focal_terms(ce, expf(-ce), alpha ? alpha[y] : 1.f, gamma, l, wgt);
    }
  }
  const float cw = wgt * inv_b;
  float kl = 0.f;
  for (int c = t; c < C; c += 256) {
    const float ls = (S[row + c] - ms) - lgs;
    const float lq = (Q[row + c] - mq) - lgq;
    const float ps = expf(ls), pq = expf(lq);
    kl = fmaf(pq, lq - ls, kl);
    G[row + c] = cw * (ps - (c == y ? 1.f : 0.f)) + klw * (ps - pq);
  }
  kl = block_reduce<false>(kl, sm);
  if (t == 0) {
    rowce[b] = l;
    rowkl[b] = kl;
  }
}

// acc[q] += sum_{k in [k0, k1)} coef(k) M[k][ec[q]], rows in order, RU of them in flight.
template <int EQ, typename F>
__device__ __forceinline__ void accum_rows(float (&acc)[EQ], const float* __restrict__ M, int E, const int (&ec)[EQ],
                                           int k0, int k1, F coef) {
  for (int k = k0; k < k1; k += RU) {
    float cf[RU], v[RU][EQ];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int kc = min(k + u, k1 - 1);
      const float c = coef(kc);
      cf[u] = k + u < k1 ? c : 0.f;
      const float* r = M + (size_t)kc * E;
#pragma unroll
      for (int q = 0; q < EQ; ++q) v[u][q] = r[ec[q]];
    }
#pragma unroll
    for (int u = 0; u < RU; ++u)
#pragma unroll
      for (int q = 0; q < EQ; ++q) acc[q] = fmaf(cf[u], v[u][q], acc[q]);
  }
}

// One wave finishes a row: g = graw + wsign sign(n - ref rref), n = x rx; out = gs rx (g - (g . n) n).
// graw(e0, ec, acc) fills the chunk's 64 EQ elements. A row of one chunk stays in registers; a
// longer one parks g in out (each lane reads back only what it wrote itself).
template <int EQ, typename FG>
__device__ __forceinline__ void project_row(int E, int lane, const float* __restrict__ x, float rx,
                                            const float* __restrict__ ref, float rref, float wsign, float gs,
                                            float* out, FG graw) {
  const bool single = E <= 64 * EQ;
  float g[EQ], n[EQ];
  float dot = 0.f;
  for (int e0 = 0; e0 < E; e0 += 64 * EQ) {
    int ec[EQ];
#pragma unroll
    for (int q = 0; q < EQ; ++q) {
      ec[q] = min(e0 + lane + 64 * q, E - 1);
      g[q] = 0.f;
    }
    graw(e0, ec, g);
#pragma unroll
    for (int q = 0; q < EQ; ++q) {
      const bool ok = e0 + lane + 64 * q < E;
      n[q] = x[ec[q]] * rx;
      g[q] += wsign * sign0(n[q] - ref[ec[q]] * rref);
      dot = fmaf(ok ? g[q] : 0.f, n[q], dot);
      if (!single && ok) out[ec[q]] = g[q];
    }
  }
  dot = wave_sum(dot);
  const float k = gs * rx;
  if (single) {
#pragma unroll
    for (int q = 0; q < EQ; ++q)
      if (lane + 64 * q < E) out[lane + 64 * q] = k * (g[q] - dot * n[q]);
    return;
  }
  for (int e = lane; e < E; e += 64) out[e] = k * (out[e] - dot * (x[e] * rx));
}

// Waves [0, C): d_txt row c. Waves after them: (image row b, C slice j) of scale G t into dpart.
template <int EQ>
__global__ __launch_bounds__(256) void grad_kernel(int B, int C, int E, int cslices, int cchunk, float scale,
                                                   float wt, float gs, const float* __restrict__ img,
                                                   const float* __restrict__ txt,
                                                   const float* __restrict__ fixed_n, const float* __restrict__ G,
                                                   const float* __restrict__ ri_img,
                                                   const float* __restrict__ ri_txt, float* __restrict__ dpart,
                                                   float* d_txt) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w < C) {
    const int c = (int)w;
    project_row<EQ>(E, lane, txt + (size_t)c * E, ri_txt[c], fixed_n + (size_t)c * E, 1.0f, wt, gs,
                    d_txt + (size_t)c * E, [&](int, const int(&ec)[EQ], float(&acc)[EQ]) {
                      accum_rows<EQ>(acc, img, E, ec, 0, B,
                                     [&](int b) { return scale * G[(size_t)b * C + c] * ri_img[b]; });
                    });
    return;
  }
  const long r = w - C;
  if (r >= (long)B * cslices) return;
  const int b = (int)(r / cslices), j = (int)(r % cslices);
  const int c0 = j * cchunk, c1 = min(C, c0 + cchunk);
  const float* grow = G + (size_t)b * C;
  float* out = dpart + ((size_t)j * B + b) * E;
  for (int e0 = 0; e0 < E; e0 += 64 * EQ) {
    int ec[EQ];
    float acc[EQ];
#pragma unroll
    for (int q = 0; q < EQ; ++q) {
      ec[q] = min(e0 + lane + 64 * q, E - 1);
      acc[q] = 0.f;
    }
    accum_rows<EQ>(acc, txt, E, ec, c0, c1, [&](int c) { return scale * grow[c] * ri_txt[c]; });
#pragma unroll
    for (int q = 0; q < EQ; ++q)
      if (e0 + lane + 64 * q < E) out[e0 + lane + 64 * q] = acc[q];
  }
}

// loss[0..4] = total, ce, kl, l1_text, l1_image by one wave: lane l sums rows l, l + 64, ... in
// order, then the butterfly.
__device__ __forceinline__ float strided_sum(int n, int lane, const float* __restrict__ v) {
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += v[i];
  return wave_sum(s);
}

__device__ __forceinline__ void loss_reduce(int B, int C, int lane, const float* __restrict__ rowce,
                                            const float* __restrict__ rowkl, const float* __restrict__ l1t,
                                            const float* __restrict__ l1i, float inv_b, float klw, float wt,
                                            float wi, float* __restrict__ loss) {
  const float ce = strided_sum(B, lane, rowce) * inv_b;
  const float kl = strided_sum(B, lane, rowkl) * klw;
  const float lt = strided_sum(C, lane, l1t) * wt;
  const float li = strided_sum(B, lane, l1i) * wi;
  if (lane == 0) {
    loss[0] = ((ce + kl) + lt) + li;
    loss[1] = ce;
    loss[2] = kl;
    loss[3] = lt;
    loss[4] = li;
  }
}

__global__ __launch_bounds__(64) void loss_kernel(int B, int C, const float* __restrict__ rowce,
                                                  const float* __restrict__ rowkl, const float* __restrict__ l1t,
                                                  const float* __restrict__ l1i, float inv_b, float klw, float wt,
                                                  float wi, float* __restrict__ loss) {
  loss_reduce(B, C, threadIdx.x, rowce, rowkl, l1t, l1i, inv_b, klw, wt, wi, loss);
}

// Waves [0, B): d_img row b from the C slices of dpart, summed in slice order. The block after them
// holds the loss sums.
template <int EQ>
__global__ __launch_bounds__(256) void image_kernel(int B, int C, int E, int cslices, float wi, float gs,
                                                    const float* __restrict__ img, const float* __restrict__ zs,
                                                    const float* __restrict__ dpart,
                                                    const float* __restrict__ ri_img,
                                                    const float* __restrict__ ri_zs,
                                                    const float* __restrict__ rowce,
                                                    const float* __restrict__ rowkl, const float* __restrict__ l1t,
                                                    const float* __restrict__ l1i, float inv_b, float klw, float wt,
                                                    float* __restrict__ loss, float* d_img) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x < 64) loss_reduce(B, C, lane, rowce, rowkl, l1t, l1i, inv_b, klw, wt, wi, loss);
    return;
  }
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const size_t be = (size_t)B * E;
  const float* prow = dpart + (size_t)b * E;
  project_row<EQ>(E, lane, img + (size_t)b * E, ri_img[b], zs + (size_t)b * E, ri_zs[b], wi, gs,
                  d_img + (size_t)b * E, [&](int, const int(&ec)[EQ], float(&acc)[EQ]) {
                    // RU slices in flight; slices past the last are fetched clamped and added as zeros
                    for (int j0 = 0; j0 < cslices; j0 += RU) {
                      float v[RU][EQ];
#pragma unroll
                      for (int u = 0; u < RU; ++u)
#pragma unroll
                        for (int q = 0; q < EQ; ++q) v[u][q] = prow[(size_t)min(j0 + u, cslices - 1) * be + ec[q]];
#pragma unroll
                      for (int u = 0; u < RU; ++u)
#pragma unroll
                        for (int q = 0; q < EQ; ++q) acc[q] += j0 + u < cslices ? v[u][q] : 0.f;
                    }
                  });
}

bool shape_ok(int B, int C, int E) { return B >= 1 && B <= kMaxB && C >= 1 && E >= 1; }

}  // namespace

extern "C" size_t clipk_src_head_ws_bytes(int B, int C, int E) {
  if (!shape_ok(B, C, E)) return 0;
  const Plan p = make_plan(B, C, E);
  return (carve(nullptr, B, C, E, p).floats * sizeof(float) + 255) / 256 * 256;
}

extern "C" int clipk_src_head(int B, int C, int E, const float* img, const float* txt, const float* zs_img,
                              const float* fixed_n, const float* fixed_q, const int64_t* labels,
                              const float* alpha, float gamma, int focal, float scale, float w_text,
                              float w_image, float w_logits, float grad_scale, float* loss, float* logits,
                              float* d_img, float* d_txt, void* ws, void* stream) {
  if (!img || !txt || !zs_img || !fixed_n || !fixed_q || !labels || !loss || !ws) return CLIPK_EINVAL;
  if ((d_img == nullptr) != (d_txt == nullptr) || (uintptr_t)ws % sizeof(float)) return CLIPK_EINVAL;
  if (!(scale > 0.f) || (focal && !(gamma >= 0.f))) return CLIPK_EINVAL;
  if (!shape_ok(B, C, E)) return CLIPK_ESHAPE;
  const Plan p = make_plan(B, C, E);
  const Ws w = carve((float*)ws, B, C, E, p);
  hipStream_t st = (hipStream_t)stream;
  const float inv_b = 1.0f / (float)B;
  const float klw = (float)((double)w_logits / ((double)B * C));
  const float wt = (float)((double)w_text / ((double)C * E));
  const float wi = (float)((double)w_image / ((double)B * E));
  const long nrows = ((long)B + C + 3) / 4;
  if (p.nprod + nrows > 0x7fffffffL || ((long)C + (long)B * p.cslices + 3) / 4 > 0x7fffffffL) return CLIPK_ESHAPE;
  hipLaunchKernelGGL(dots_kernel, dim3((unsigned)(p.nprod + nrows)), dim3(256), 0, st, B, C, E, p.tb, p.tc, p.splits,
                     p.kchunk, p.nprod, img, txt, zs_img, fixed_n, fixed_q, w.part, w.ri_img, w.ri_zs, w.ri_txt,
                     w.l1i, w.l1t);
  CLIPK_CHECK_LAUNCH();
  float* S = logits ? logits : w.S;
  hipLaunchKernelGGL(rows_kernel, dim3(B), dim3(256), 0, st, B, C, p.splits, scale, w.part, w.ri_img, w.ri_zs,
                     w.ri_txt, labels, alpha, gamma, focal, inv_b, klw, S, w.Q, w.G, w.rowce, w.rowkl);
  CLIPK_CHECK_LAUNCH();
  if (!d_img) {
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(64), 0, st, B, C, w.rowce, w.rowkl, w.l1t, w.l1i, inv_b, klw, wt,
                       wi, loss);
    CLIPK_CHECK_LAUNCH();
    return CLIPK_OK;
  }
  const dim3 ggrid((unsigned)(((long)C + (long)B * p.cslices + 3) / 4));
  const dim3 igrid((B + 3) / 4 + 1);
#define CLIPK_SRC_GRAD(EQ)                                                                                          \
  do {                                                                                                              \
    hipLaunchKernelGGL(grad_kernel<EQ>, ggrid, dim3(256), 0, st, B, C, E, p.cslices, p.cchunk, scale, wt,           \
                       grad_scale, img, txt, fixed_n, w.G, w.ri_img, w.ri_txt, w.dpart, d_txt);                     \
    CLIPK_CHECK_LAUNCH();                                                                                           \
    hipLaunchKernelGGL(image_kernel<EQ>, igrid, dim3(256), 0, st, B, C, E, p.cslices, wi, grad_scale, img, zs_img,  \
                       w.dpart, w.ri_img, w.ri_zs, w.rowce, w.rowkl, w.l1t, w.l1i, inv_b, klw, wt, loss, d_img);    \
    CLIPK_CHECK_LAUNCH();                                                                                           \
  } while (0)
  // elements per lane and chunk: a row of E <= 64 EQ stays in registers
  if (E <= 256) CLIPK_SRC_GRAD(4);
  else if (E <= 512) CLIPK_SRC_GRAD(8);
  else CLIPK_SRC_GRAD(12);
#undef CLIPK_SRC_GRAD
  return CLIPK_OK;
}
