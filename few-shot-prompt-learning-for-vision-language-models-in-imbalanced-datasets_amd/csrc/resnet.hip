// ModifiedResNet forward (PromptSRC/clip/model.py:94-150) as one launch sequence over the
// convolution kernels of conv.hip, behind an opaque handle holding host-side pointers to the
// caller's packed weights. Frozen and forward-only; all launches go to the caller's stream, no
// allocation, no host sync.
#include <algorithm>
#include <new>
#include <vector>

#include "common.h"

struct clipk_resnet {
  int width, blocks[4], embed, res, act;
  std::vector<const void*> p;
};

namespace clipk {

static inline size_t rn_up(size_t x) { return (x + 255) & ~size_t(255); }

// The feature maps of one forward, in elements: the stem's gather and three maps, then per block
// its input / output (ping-pong), conv1 and conv2 outputs, the two pooled maps and the identity.
struct RnPlan {
  size_t gather, io, t1, t2, pool, xpool, id;
};

static RnPlan rn_plan(const clipk_resnet* h, size_t B) {
  RnPlan p{};
  const size_t w = h->width;
  size_t s = h->res / 2;
  p.gather = B * s * s * 32;
  p.t1 = B * s * s * (w / 2);  // stem conv1 / conv2 outputs share the block buffers
  p.t2 = B * s * s * (w / 2);
  p.io = B * s * s * w;  // stem conv3 output
  s /= 2;
  p.io = std::max(p.io, B * s * s * w);
  size_t inpl = w;
  for (int l = 0; l < 4; ++l) {
    const size_t planes = w << l;
    for (int i = 0; i < h->blocks[l]; ++i) {
      const bool stride = l > 0 && i == 0;
      p.t1 = std::max(p.t1, B * s * s * planes);
      p.t2 = std::max(p.t2, B * s * s * planes);
      if (stride) {
        p.pool = std::max(p.pool, B * (s / 2) * (s / 2) * planes);
        p.xpool = std::max(p.xpool, B * (s / 2) * (s / 2) * inpl);
        s /= 2;
      }
      if (i == 0) p.id = std::max(p.id, B * s * s * planes * 4);
      p.io = std::max(p.io, B * s * s * planes * 4);
      inpl = planes * 4;
    }
  }
  return p;
}

}  // namespace clipk

using namespace clipk;

extern "C" int clipk_resnet_create(int width, const int* blocks, int embed, int res, int act_dtype,
                                   const void* const* ptrs, int n_ptrs, clipk_resnet** out) {
  if (!blocks || !ptrs || !out) return CLIPK_EINVAL;
  if (act_dtype != CLIPK_F32 && act_dtype != CLIPK_F16 && act_dtype != CLIPK_BF16) return CLIPK_EINVAL;
  if (width <= 0 || width % 64 || embed <= 0 || embed % 32 || res <= 0 || res % 32) return CLIPK_EINVAL;
  const int S = res / 32;
  if (S * S + 1 > 256) return CLIPK_EINVAL;
  int nb = 0;
  for (int l = 0; l < 4; ++l) {
    if (blocks[l] <= 0) return CLIPK_EINVAL;
    nb += blocks[l];
  }
  if (n_ptrs != 9 + 12 * nb + 7) return CLIPK_EINVAL;
  // every pointer but a block's absent downsample is required; a layer's first block has one
  int k = 9;
  for (int i = 0; i < 9; ++i)
    if (!ptrs[i]) return CLIPK_EINVAL;
  for (int l = 0; l < 4; ++l)
    for (int i = 0; i < blocks[l]; ++i, k += 12) {
      for (int j = 0; j < 9; ++j)
        if (!ptrs[k + j]) return CLIPK_EINVAL;
      const bool ds = ptrs[k + 9] != nullptr;
      if (ds != (ptrs[k + 10] != nullptr) || ds != (ptrs[k + 11] != nullptr) || ds != (i == 0)) return CLIPK_EINVAL;
    }
  for (int i = 0; i < 7; ++i)
    if (!ptrs[k + i]) return CLIPK_EINVAL;
  clipk_resnet* h = new (std::nothrow) clipk_resnet;
  if (!h) return CLIPK_EINVAL;
  h->width = width;
  for (int l = 0; l < 4; ++l) h->blocks[l] = blocks[l];
  h->embed = embed;
  h->res = res;
  h->act = act_dtype;
  h->p.assign(ptrs, ptrs + n_ptrs);
  *out = h;
  return CLIPK_OK;
}

extern "C" void clipk_resnet_destroy(clipk_resnet* h) { delete h; }

extern "C" size_t clipk_resnet_ws_bytes(const clipk_resnet* h, int B) {
  if (!h || B <= 0) return 0;
  const RnPlan p = rn_plan(h, (size_t)B);
  const size_t e = h->act == CLIPK_F32 ? 4 : 2;
  const int S = h->res / 32;
  return rn_up(p.gather * e) + 2 * rn_up(p.io * e) + rn_up(p.t1 * e) + rn_up(p.t2 * e) + rn_up(p.pool * e) +
         rn_up(p.xpool * e) + rn_up(p.id * e) + clipk_attnpool_ws_bytes(h->act, B, S * S, 32 * h->width);
}

#define RN_TRY(call)        \
  do {                      \
    const int _rc = (call); \
    if (_rc) return _rc;    \
  } while (0)

extern "C" int clipk_resnet_forward(const clipk_resnet* h, int B, const float* img, float* feat, void* ws,
                                    size_t ws_bytes, void* stream) {
  if (!h || !img || !feat || B < 0) return CLIPK_EINVAL;
  if (B == 0) return CLIPK_OK;
  if (!ws || ((uintptr_t)ws & 255)) return CLIPK_EINVAL;
  if (ws_bytes < clipk_resnet_ws_bytes(h, B)) return CLIPK_EWORKSPACE;
  const RnPlan pl = rn_plan(h, (size_t)B);
  const size_t e = h->act == CLIPK_F32 ? 4 : 2;
  char* c = (char*)ws;
  auto take = [&](size_t elems) {
    void* q = c;
    c += rn_up(elems * e);
    return q;
  };
  void* gather = take(pl.gather);
  void* io[2] = {take(pl.io), take(pl.io)};
  void* t1 = take(pl.t1);
  void* t2 = take(pl.t2);
  void* pool = take(pl.pool);
  void* xpool = take(pl.xpool);
  void* idb = take(pl.id);
  void* aws = c;
  const int dt = h->act, w = h->width;
  const void* const* p = h->p.data();
  const float* const* pf = reinterpret_cast<const float* const*>(p);
  const int RELU = CLIPK_CONV_RELU;

  // stem: three conv + BatchNorm + ReLU, then AvgPool2d(2)
  int s = h->res / 2;
  RN_TRY(clipk_im2col_3x3s2(dt, B, h->res, img, gather, stream));
  RN_TRY(clipk_conv2d_nhwc(dt, RELU, B, s, s, 32, w / 2, 1, gather, p[0], pf[1], pf[2], nullptr, t1, stream));
  RN_TRY(clipk_conv2d_nhwc(dt, RELU, B, s, s, w / 2, w / 2, 3, t1, p[3], pf[4], pf[5], nullptr, t2, stream));
  RN_TRY(clipk_conv2d_nhwc(dt, RELU, B, s, s, w / 2, w, 3, t2, p[6], pf[7], pf[8], nullptr, io[1], stream));
  RN_TRY(clipk_avgpool2_nhwc(dt, B, s, s, w, io[1], io[0], stream));
  s /= 2;

  int cur = 0, inpl = w, k = 9;
  for (int l = 0; l < 4; ++l) {
    const int planes = w << l;
    for (int i = 0; i < h->blocks[l]; ++i, k += 12) {
      const bool stride = l > 0 && i == 0;
      const void* x = io[cur];
      void* y = io[cur ^ 1];
      RN_TRY(clipk_conv2d_nhwc(dt, RELU, B, s, s, inpl, planes, 1, x, p[k], pf[k + 1], pf[k + 2], nullptr, t1, stream));
      RN_TRY(clipk_conv2d_nhwc(dt, RELU, B, s, s, planes, planes, 3, t1, p[k + 3], pf[k + 4], pf[k + 5], nullptr, t2,
                               stream));
      const void* main_in = t2;
      const void* id_in = x;
      if (stride) {
        RN_TRY(clipk_avgpool2_nhwc(dt, B, s, s, planes, t2, pool, stream));
        RN_TRY(clipk_avgpool2_nhwc(dt, B, s, s, inpl, x, xpool, stream));
        main_in = pool;
        id_in = xpool;
        s /= 2;
      }
      const void* id = x;
      if (p[k + 9]) {
        RN_TRY(clipk_conv2d_nhwc(dt, 0, B, s, s, inpl, planes * 4, 1, id_in, p[k + 9], pf[k + 10], pf[k + 11], nullptr,
                                 idb, stream));
        id = idb;
      }
      RN_TRY(clipk_conv2d_nhwc(dt, CLIPK_CONV_RES | RELU, B, s, s, planes, planes * 4, 1, main_in, p[k + 6], pf[k + 7],
                               pf[k + 8], id, y, stream));
      cur ^= 1;
      inpl = planes * 4;
    }
  }
  const size_t used = (size_t)((char*)aws - (char*)ws);
  return clipk_attnpool(dt, B, s * s, inpl, inpl / 64, h->embed, io[cur], pf[k], p[k + 1], pf[k + 2], p[k + 3],
                        pf[k + 4], p[k + 5], pf[k + 6], feat, aws, ws_bytes - used, stream);
}
