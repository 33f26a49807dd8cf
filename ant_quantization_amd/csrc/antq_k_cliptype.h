// antq_k_cliptype.h -- what the clip searches that treat the quantiser as a step function of x share: a codebook's descriptor,
// an element's fixed-point image and the literal (reference-sequence) evaluation of an element that is no step-function element.
// Part of libantq's calibration translation unit; used by the sorted-row search (antq_k_sortsearch.h) and by the threshold
// sweep (antq_k_sweep.h), which do not include each other.  gfx950 only.
#ifndef ANTQ_K_CLIPTYPE_H
#define ANTQ_K_CLIPTYPE_H

#include "antq_device.h"

namespace antq {

struct ClipType {
    const uint4 *tlist;      // device: HThr[n_thr]
    const float *grid;       // device: the codebook in scan order (literal path)
    uint32_t n_thr, m;
    float gmax, lim;         // lim: |x / s| below this -> the step function is the whole story (HArgs::lim)
    int kout_pos, kout_neg;  // OliVe: the threshold between the last normal value and the first outlier, per sign (-1: none)
};

// the reference sequence for one element at one scale (quant_kernel.cu:25-37 scan, AQ:541-549): q before any pair rule
__device__ __forceinline__ float clip_literal_q(float xv, float s, const float *__restrict__ grid, int m, float &d)
{
    d = xv / s;
    float sub_min = 102400.0f, z_min = 0.0f;
#pragma unroll 1
    for (int i = 0; i < m; i++) {
        const float g = grid[i];
        const float sub_v = fabsf(d - g);
        if (sub_v <= sub_min) { sub_min = sub_v; z_min = g; }
    }
    return z_min;
}
__device__ __forceinline__ double clip_literal_term(float q, float d, float s, float xv)
{
    const float tt = (q - d) + d;
    const float df = fabsf(tt * s - xv);
    // widened BEFORE squaring: a literal element's term is as exact as the closed form's terms around it (squared in float, a
    // far-clipped element -- the largest term of its row -- carried a 2^-24 rounding into the row's sum, and 1e30 gave Inf)
    return (double)df * (double)df;
}

// x in fixed point, units of 2^(ex - 38), as a 64-bit integer: |x| < 2^(ex + 8) -> |x * F| < 2^46, so adding 1.5 * 2^52 leaves
// rint(x * F) in the low 52 bits of the double (round to nearest even: one fixed rule -- every run forms the same integer)
__device__ __forceinline__ long long clip_fixed(float xv, double F)
{
    const double d = (double)xv * F + 6755399441055744.0;
    return (long long)(__double_as_longlong(d) & 0x000fffffffffffffll) - 0x0008000000000000ll;
}

}  // namespace antq

#endif  // ANTQ_K_CLIPTYPE_H
