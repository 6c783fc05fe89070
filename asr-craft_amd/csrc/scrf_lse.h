// scrf_lse.h -- workgroup-wide column log-sum-exp of the log-domain workgroup kernels (k_fb, k_fb_segtrans):
// max-shifted like the reference's logAdd(double*, double max, int) (utils/CRF_LogMath.cpp:102-125).
#ifndef SCRF_LSE_H_
#define SCRF_LSE_H_

#include "scrf_common.h"

struct FbLse {
  int L, G, g, j;
  bool active;
  double* red_m;
  double* red_s;
};

template <class VAL>
__device__ __forceinline__ double col_lse(const FbLse& c, int n_i, VAL val, int* err) {
  // returns LSE_i val(i, j) to the threads of group 0 (others get garbage); 3 barriers
  double m = -INFINITY;
  if (c.active)
    for (int i = c.g; i < n_i; i += c.G) m = fmax(m, val(i, c.j, true));
  if (c.active) c.red_m[c.g * c.L + c.j] = m;
  __syncthreads();
  double mm = -INFINITY, s = 0.0;
  if (c.active) {
    for (int gg = 0; gg < c.G; gg++) mm = fmax(mm, c.red_m[gg * c.L + c.j]);
    for (int i = c.g; i < n_i; i += c.G) s += exp(val(i, c.j, false) - mm);
    c.red_s[c.g * c.L + c.j] = s;
  }
  __syncthreads();
  double r = 0.0;
  if (c.active && c.g == 0) {
    double tot = 0.0;
    for (int gg = 0; gg < c.G; gg++) tot += c.red_s[gg * c.L + c.j];
    if (!(tot > 0.0) || isinf(tot) || isnan(tot)) *err = SCRF_ERR_NUMERIC;  // logE(0) / NaN / Inf
    r = mm + log(tot);
  }
  return r;
}

// One thread's max-shifted log-sum-exp over terms given one by one, in the caller's order (scrf_transcript.hip): the shift
// follows the running maximum, so every term costs one exp and none is evaluated twice.  -inf terms are skipped; no term
// at all gives -inf; a NaN term gives NaN.
struct LseAcc {
  double m = -INFINITY, s = 0.0;
  __device__ __forceinline__ void add(double x) {
    if (x == -INFINITY) return;
    if (x > m) { s = s * exp(m - x) + 1.0; m = x; }
    else s += exp(x - m);
  }
  __device__ __forceinline__ double value() const { return (s > 0.0 || s != s) ? m + log(s) : -INFINITY; }
};

#endif  // SCRF_LSE_H_
