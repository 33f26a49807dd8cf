// antq_k_linear4.h -- y = x . W^T (+ bias) for 1 .. 8 rows of x, straight from the packed 4-bit codes of W (antq_linear4)
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// With few rows of x a linear layer is a weight stream: every weight is used M times and never again.  The codes are a
// quarter of the bf16 image's bytes, so the kernel streams them and makes the image's values on the fly -- through the
// decoder's own byte table (antq_k_decbatch.h: dec_pair / DecOut), so that W[n, k] IS the element antq_decode4 writes.
//
//   ownership  one-wavefront workgroups, no barrier, no shared state; a wavefront owns R consecutive output rows over the
//              whole of K (R = 2 for M <= 2, 4 beyond: more wavefronts where the kernel is a stream, more reuse of the
//              unpacked x where it is arithmetic)
//   loads      codes straight to VGPRs, nontemporal, 16 B (VEC: 32 elements) or 4 B (8 elements) per lane and row, the
//              next step's in flight while this one is computed; x is re-read by every wavefront and lives in L2: plain
//              cached 16-byte loads, one step ahead as well where that costs few registers (M <= 2; fp32: M = 1)
//   decode     a wave-private table of 256 entries per row (per tensor: one), keyed by the code BYTE, entry = the pair's two
//              finished outputs in the output type; per pair one ds_read_b32 (bf16 / f16) or ds_read_b64 (fp32) and the
//              exact widening to fp32
//   sum        acc[m][r] = fmaf(x, w, acc) in fp32, lane l over its own k in rising order; then ONE cross-lane reduction in
//              a fixed pattern: four DPP steps inside each row of 16 lanes, the four row sums as (r0 + r1) + (r2 + r3).
//              The sequence of operations that makes y[m, n] depends on K and on the alignment of the codes only -- not on
//              M, not on the other rows of x, not on R: a row computed alone has the bits it has in a call of 8.
//   store      lane i keeps value i: bias added in fp32, rounded to the output type, one element store per lane
#ifndef ANTQ_K_LINEAR4_H
#define ANTQ_K_LINEAR4_H

#include "antq_k_decbatch.h"

namespace antq {

constexpr int lin4_rows(int M) { return M <= 2 ? 2 : 4; }      // R: output rows per wavefront

// a table entry -> the pair's two weights as fp32 (exact widening of the output type)
template <typename T> struct Lin4W;
template <> struct Lin4W<float> {
    __device__ __forceinline__ static void get(const uint2 &e, float &a, float &b) { a = u2f(e.x); b = u2f(e.y); }
};
template <> struct Lin4W<bf16_tag> {
    __device__ __forceinline__ static void get(uint32_t e, float &a, float &b) { a = u2f(e << 16); b = u2f(e & 0xffff0000u); }
};
template <> struct Lin4W<f16_tag> {
    __device__ __forceinline__ static void get(uint32_t e, float &a, float &b)
    {
        a = IO<f16_tag>::h2f(e & 0xffffu);
        b = IO<f16_tag>::h2f(e >> 16);
    }
};

// 8 consecutive elements of x (the first at a multiple of 8: 16-byte aligned) as raw vectors, and as floats
template <typename T> struct Lin4X {
    static constexpr int V = 1;
    __device__ __forceinline__ static void load(const void *x, size_t elem, uint4 (&v)[1]) { v[0] = ld_global(static_cast<const uint4 *>(x) + elem / 8); }
    __device__ __forceinline__ static void unpack(const uint4 (&v)[1], float (&f)[8]) { IO<T>::unpack(v[0], f); }
};
template <> struct Lin4X<float> {
    static constexpr int V = 2;
    __device__ __forceinline__ static void load(const void *x, size_t elem, uint4 (&v)[2])
    {
        const uint4 *p = static_cast<const uint4 *>(x) + elem / 4;
        v[0] = ld_global(p);
        v[1] = ld_global(p + 1);
    }
    __device__ __forceinline__ static void unpack(const uint4 (&v)[2], float (&f)[8])
    {
        f[0] = u2f(v[0].x); f[1] = u2f(v[0].y); f[2] = u2f(v[0].z); f[3] = u2f(v[0].w);
        f[4] = u2f(v[1].x); f[5] = u2f(v[1].y); f[6] = u2f(v[1].z); f[7] = u2f(v[1].w);
    }
};

template <int CTRL>
__device__ __forceinline__ float lin4_dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// the sum over the 64 lanes, the same tree for every value; all lanes active
__device__ __forceinline__ float lin4_wave_sum(float v)
{
    v += lin4_dpp<0xB1>(v);                             // quad_perm [1,0,3,2]
    v += lin4_dpp<0x4E>(v);                             // quad_perm [2,3,0,1]
    v += lin4_dpp<0x141>(v);                            // row_half_mirror
    v += lin4_dpp<0x140>(v);                            // row_mirror: every lane of a row of 16 holds the row's sum
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

// M: rows of x the kernel computes (rows >= m_rows repeat the last one and are not stored); VEC: 16 B of codes per lane
template <typename T, bool OVP, int M, bool VEC>
__global__ void __launch_bounds__(64)
k_linear4(const uint32_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
          uint32_t m_rows, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
          const float *__restrict__ grid, uint32_t m, int n_normal)
{
    typedef typename DecOut<T>::Ent Ent;
    constexpr int R = lin4_rows(M);
    constexpr int W = VEC ? 4 : 1;                     // code words (8 elements each) per lane, row and step
    constexpr int XV = Lin4X<T>::V;
    constexpr bool XP = M * XV <= 2;                   // x one step ahead in registers too (where that is few registers)
    __shared__ __attribute__((aligned(16))) Ent tab[R * 256];
    __shared__ float g[32];
    const uint32_t lane = threadIdx.x;
    const uint32_t row0 = __builtin_amdgcn_readfirstlane(blockIdx.x) * (uint32_t)R;
    const uint32_t wpr = K >> 3;                       // code words per row
    const uint32_t gpr = wpr / W;                      // a lane's load units per row (VEC: K % 32 == 0)
    const uint32_t steps = (gpr + 63u) >> 6;
    const ANTQ_GLOBAL uint32_t *crow[R];
    const char *xrow[M];
#pragma unroll
    for (int r = 0; r < R; r++) crow[r] = (const ANTQ_GLOBAL uint32_t *)(codes) + (size_t)min(row0 + r, N - 1u) * wpr;
#pragma unroll
    for (int i = 0; i < M; i++) xrow[i] = static_cast<const char *>(x) + (size_t)min((uint32_t)i, m_rows - 1u) * K * IO<T>::ESIZE;   // (the 16-bit tags are empty types)

    uint32_t cw[R][W], nw[R][W];
    uint4 xc[XP ? M : 1][W][XV], xn[XP ? M : 1][W][XV];
    auto load_step = [&](uint32_t s, uint32_t (&w)[R][W], uint4 (&xs)[XP ? M : 1][W][XV]) {
        const uint32_t u = min(s * 64u + lane, gpr - 1u);          // (lanes past the row's end repeat its last unit, unused)
#pragma unroll
        for (int r = 0; r < R; r++) {
            if constexpr (VEC) {
                const u32x4_t v = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(crow[r]) + u);
                w[r][0] = v.x; w[r][1] = v.y; w[r][2] = v.z; w[r][3] = v.w;
            } else w[r][0] = __builtin_nontemporal_load(crow[r] + u);
        }
        if constexpr (XP) {
#pragma unroll
            for (int i = 0; i < M; i++)
#pragma unroll
                for (int j = 0; j < W; j++) Lin4X<T>::load(xrow[i], ((size_t)u * W + j) * 8u, xs[i][j]);
        }
    };
    load_step(0u, cw, xc);                              // in flight while the tables are built

    // (+ 0.0f: a codebook's -0 decodes to +0, as in the decoders)
    if (lane < 32u) g[lane] = (lane < m) ? ld_global(grid + lane) + 0.0f : 0.0f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t tstride = per_row ? 256u : 0u;      // one scale per tensor: one table
    for (int r = 0; r < (per_row ? R : 1); r++) {
        const float a = ld_global(alpha + (per_row ? min(row0 + r, N - 1u) : 0u));
        const float s = a / gmax;                       // AQ:536 scale = alpha / max(grid)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t b = lane + 64u * k;
            float q0, q1;
            dec_pair<OVP>(b, g, n_normal, q0, q1);
            tab[r * 256 + b] = DecOut<T>::make(q0 * s, q1 * s);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    float acc[M][R];
#pragma unroll
    for (int i = 0; i < M; i++)
#pragma unroll
        for (int r = 0; r < R; r++) acc[i][r] = 0.0f;

    for (uint32_t s = 0; s < steps; s++) {
        const bool more = s + 1u < steps;
        if (more) load_step(s + 1u, nw, xn);
        const uint32_t u = s * 64u + lane;
        if (u < gpr) {
#pragma unroll
            for (int j = 0; j < W; j++) {
                float xf[M][8];
#pragma unroll
                for (int i = 0; i < M; i++) {
                    if constexpr (XP) Lin4X<T>::unpack(xc[i][j], xf[i]);
                    else {
                        uint4 xv[XV];
                        Lin4X<T>::load(xrow[i], ((size_t)u * W + j) * 8u, xv);
                        Lin4X<T>::unpack(xv, xf[i]);
                    }
                }
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const uint32_t word = cw[r][j];
                    const Ent *t = tab + r * tstride;
                    Ent e[4];
#pragma unroll
                    for (int p = 0; p < 4; p++) e[p] = t[(word >> (8 * p)) & 0xffu];
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        float w0, w1;
                        Lin4W<T>::get(e[p], w0, w1);
#pragma unroll
                        for (int i = 0; i < M; i++) {
                            acc[i][r] = __builtin_fmaf(xf[i][2 * p], w0, acc[i][r]);
                            acc[i][r] = __builtin_fmaf(xf[i][2 * p + 1], w1, acc[i][r]);
                        }
                    }
                }
            }
        }
        if (!more) break;
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int j = 0; j < W; j++) cw[r][j] = nw[r][j];
        if constexpr (XP) {
#pragma unroll
            for (int i = 0; i < M; i++)
#pragma unroll
                for (int j = 0; j < W; j++)
#pragma unroll
                    for (int v = 0; v < XV; v++) xc[i][j][v] = xn[i][j][v];
        }
    }

    // value i * R + r ends up in lane i * R + r
    float mine = 0.0f;
#pragma unroll
    for (int i = 0; i < M; i++)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float t = lin4_wave_sum(acc[i][r]);
            if (lane == (uint32_t)(i * R + r)) mine = t;
        }
    const uint32_t i = lane / (uint32_t)R, r = lane % (uint32_t)R, row = row0 + r;
    if (i < m_rows && i < (uint32_t)M && row < N) {
        if (bias) mine += IO<T>::load1(bias, row);
        IO<T>::store1(y, (size_t)i * N + row, mine);
    }
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR4_H
