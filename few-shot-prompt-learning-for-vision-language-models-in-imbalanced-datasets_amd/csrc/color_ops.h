// Per-pixel arithmetic of the colour stage (preprocess.hip, clipk_image_color): torchvision's
// ColorJitter / RandomGrayscale on PIL images, restated so that every uint8 result is Pillow's
// (libImaging Blend.c, Convert.c rgb2hsv_row / hsv2rgb / L24). Plain C++ with no device builtins:
// the same functions compile for the host, where they can be swept over all 2^24 RGB triples.
//
// Precisions are Pillow's and matter: the blend's multiply and add round separately in fp32 (a
// fused multiply-add differs in ~10^5 of the 2^24 triples at f = 0.6); RGB -> HSV mixes fp32 and
// double exactly as the C source does; HSV -> RGB is fp32 throughout. Contraction is switched off
// in every function, and the divisions are the correctly rounded ones (no fast-math).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CLIPK_COLOR_FN __host__ __device__ __forceinline__
#else
#define CLIPK_COLOR_FN inline
#endif

namespace clipk {
namespace color {

// ImagingConvert RGB -> L (Convert.c L24): exact over all triples.
CLIPK_COLOR_FN int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate, img, f) on one channel (ImageEnhance.*.enhance): d + f * (x - d) in fp32,
// truncated toward zero and clipped to 0..255.
CLIPK_COLOR_FN int blend(int d, int x, float f) {
#pragma clang fp contract(off)
  const float prod = f * (float)(x - d);
  const float t = (float)d + prod;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

CLIPK_COLOR_FN int clip8i(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert("HSV"), h = (h + shift) & 255, convert("RGB") on one pixel.
CLIPK_COLOR_FN void hue_shift(int& r, int& g, int& b, int shift) {
#pragma clang fp contract(off)
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  if (minc == maxc) return;  // h = s = 0: grey at v, whatever the shift
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr;
  const float gc = (float)(maxc - g) / cr;
  const float bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) {
    h = bc - gc;
  } else if (g == maxc) {
    h = (float)(2.0 + (double)rc - (double)bc);
  } else {
    h = (float)(4.0 + (double)gc - (double)rc);
  }
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  const int uh = (clip8i((int)((double)h * 255.0)) + shift) & 255;
  const int us = clip8i((int)((double)s * 255.0));
  const int v = maxc;
  if (us == 0) {
    r = g = b = v;
    return;
  }
  float f = (float)uh * 6.0f / 255.0f;
  const float fi = floorf(f);
  const int i = (int)fi;
  f = f - fi;
  const float fs = (float)us / 255.0f;
  const float fv = (float)v;
  const int p = clip8i((int)roundf(fv * (1.0f - fs)));
  const int q = clip8i((int)roundf(fv * (1.0f - fs * f)));
  const int t = clip8i((int)roundf(fv * (1.0f - fs * (1.0f - f))));
  switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// ---- Gaussian blur (ImageFilter.GaussianBlur: libImaging BoxBlur.c, three box passes per axis) ----
// One output of a box pass of integer radius r: acc = the 2r + 1 window samples summed, far = the two
// samples just outside it, ww / fw their 24-bit fixed-point weights ((2r + 1) * ww + 2 * fw <= 2^24,
// so the sum stays below 255 * 2^24 + 2^23 < 2^32).
CLIPK_COLOR_FN uint32_t box_px(uint32_t acc, uint32_t far, uint32_t ww, uint32_t fw) {
  return (acc * ww + far * fw + (1u << 23)) >> 24;
}

// One box pass over the line p[0], p[stride], ..., p[(n - 1) * stride], in place; edges repeat the
// edge sample (also when r + 1 >= n). 0 <= r <= 7. The window slides: the samples behind x that the
// line no longer holds (x - 8 .. x, already overwritten or about to be) ride in `hist`, byte k =
// in[x - k], and `old` = in[x - 8]; the samples ahead are read from the line, which is still input
// there. Started on in[0] everywhere, the history is the left edge rule.
CLIPK_COLOR_FN void box_line(uint8_t* p, int n, int stride, int r, uint32_t ww, uint32_t fw) {
  const uint32_t first = p[0];
  uint64_t hist = first * 0x0101010101010101ull;
  uint32_t old = first;
  uint32_t acc = (uint32_t)(r + 1) * first;
  for (int d = 1; d <= r; ++d) acc += p[(size_t)(d < n ? d : n - 1) * stride];
  for (int x = 0; x < n; ++x) {
    uint8_t* px = p + (size_t)x * stride;
    old = (uint32_t)(hist >> 56);
    hist = (hist << 8) | *px;
    const int xr = x + r + 1;
    const uint32_t right = p[(size_t)(xr < n ? xr : n - 1) * stride];
    const uint32_t left = r < 7 ? (uint32_t)(hist >> (8 * (r + 1))) & 255u : old;
    *px = (uint8_t)box_px(acc, left + right, ww, fw);
    acc += right - ((uint32_t)(hist >> (8 * r)) & 255u);  // window of x + 1
  }
}

}  // namespace color
}  // namespace clipk
