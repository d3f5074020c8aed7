// Coefficient arithmetic of the resample tables (preprocess.hip, clipk_resample_tables): Pillow's
// precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for the bicubic filter
// (a = -0.5, support 2, PRECISION_BITS = 22), restated for ONE output index so that every int32 is
// the one fsp_amd/data/preprocess.py resample_coeffs gives. Plain C++ with no device builtins: the
// same functions compile for the host (clipk_resample_tables_host), where the CPU tests sweep them.
//
// Every step is in double and in Pillow's order: scale, filterscale, support, ss, center; xmin and
// xmax by C truncation and their clamps; the tap weights; their sum, one tap after another in tap
// order from 0.0 (the order is part of the result); the division by the sum when it is nonzero;
// (int)(+-0.5 + w * 2^22). Contraction is switched off in every function that does float
// arithmetic, and the divisions are the correctly rounded ones (no fast-math). A row's weights are
// evaluated twice (once for the sum, once for the output) instead of being kept: ksize has no bound
// (2,797 for 699 -> 1), and the same expression on the same operands gives the same double.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CLIPK_RESAMPLE_FN __host__ __device__ __forceinline__
#else
#define CLIPK_RESAMPLE_FN inline
#endif

namespace clipk {
namespace resample {

constexpr int kPrecisionBits = 32 - 8 - 2;

// What one axis shares over its outputs: in_size -> out_size.
struct Axis {
  double scale, support, ss;
  int in_size, ksize;
};

CLIPK_RESAMPLE_FN Axis make_axis(int in_size, int out_size) {
#pragma clang fp contract(off)
  Axis a;
  a.in_size = in_size;
  a.scale = (double)in_size / (double)out_size;
  const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = 2.0 * filterscale;
  a.ss = 1.0 / filterscale;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  return a;
}

// Pillow's bicubic_filter.
CLIPK_RESAMPLE_FN double bicubic(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// One output's taps: the first source index and how many.
struct Taps {
  double center;
  int xmin, xmax;
};

CLIPK_RESAMPLE_FN Taps taps_of(const Axis& a, int xx) {
#pragma clang fp contract(off)
  Taps t;
  t.center = ((double)xx + 0.5) * a.scale;
  int xmin = (int)(t.center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(t.center + a.support + 0.5);
  if (xmax > a.in_size) xmax = a.in_size;
  t.xmin = xmin;
  t.xmax = xmax - xmin;
  return t;
}

CLIPK_RESAMPLE_FN double weight(const Axis& a, const Taps& t, int x) {
#pragma clang fp contract(off)
  return bicubic(((double)(x + t.xmin) - t.center + 0.5) * a.ss);
}

// The sum Pillow divides by: tap after tap, from 0.0.
CLIPK_RESAMPLE_FN double weight_sum(const Axis& a, const Taps& t) {
#pragma clang fp contract(off)
  double ww = 0.0;
  for (int x = 0; x < t.xmax; ++x) ww += weight(a, t, x);
  return ww;
}

// normalize_coeffs_8bpc on one normalised weight.
CLIPK_RESAMPLE_FN int fixed_coeff(double w, double ww) {
#pragma clang fp contract(off)
  if (ww != 0.0) w = w / ww;
  const double p = w * (double)(1 << kPrecisionBits);
  return w < 0 ? (int)(-0.5 + p) : (int)(0.5 + p);
}

// One table row for output xx: (first tap - first_rel, taps used, ksize coefficients, zero past
// the taps used). stride_k: the row's coefficient slots (the caller's ksize; never fewer than the
// row's taps when it is the axis's, and no slot past it is written either way). A stride_k below
// the axis's ksize therefore TRUNCATES the row (fewer taps, their sum taken over those alone)
// instead of reporting anything: the device entry cannot read its records on the host, so only
// clipk_resample_tables_host checks ksize, and a direct caller of the device entry with a wrong
// ksize gets truncated rows, not an error.
CLIPK_RESAMPLE_FN void table_row(const Axis& a, int xx, int first_rel, int stride_k, int* row) {
  Taps t = taps_of(a, xx);
  if (t.xmax > stride_k) t.xmax = stride_k;
  if (t.xmax < 0) t.xmax = 0;
  const double ww = weight_sum(a, t);
  row[0] = t.xmin - first_rel;
  row[1] = t.xmax;
  for (int x = 0; x < stride_k; ++x) row[2 + x] = x < t.xmax ? fixed_coeff(weight(a, t, x), ww) : 0;
}

}  // namespace resample
}  // namespace clipk
