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

}  // namespace color
}  // namespace clipk
