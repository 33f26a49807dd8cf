// antq_k_linear4_mm.h -- y = x . W^T (+ bias) for 1 .. 64 rows of x on the matrix cores, straight from the packed 4-bit codes
// of W (antq_linear4_mm; bf16 and f16).  Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// Beyond a handful of rows the arithmetic of a packed linear belongs on the matrix cores, and antq_encode4's layout fits
// v_mfma_f32_16x16x32_{bf16,f16}: the B fragment of lane l is B[k = 8 (l >> 4) + j][col l & 15], j = 0 .. 7 -- 8 consecutive k
// of ONE weight row, which is one 32-bit code word.  The decoder's byte table (antq_k_decbatch.h: dec_pair / DecOut) holds,
// per code byte, the pair's two finished outputs in the output type, so four ds_read_b32 look-ups ARE the four operand
// registers: W[n, k] is the element antq_decode4 writes, with no shuffle, no widening and no multiply.
//
//   ownership  workgroups of 8 wavefronts; a workgroup owns 16 NT consecutive output rows n (NT = 1 / 2 / 4, the launcher's
//              choice from M and N) for all MT = 1 / 2 / 4 tiles of 16 rows of x.  K is cut into chunks of 128 elements (VEC:
//              16 B of codes per lane) or 32 (4 B per lane); wavefront w takes chunks w, w + 8, w + 16, ... in rising order:
//              the split is a function of K and of the code path alone.
//   loads      codes straight to VGPRs, nontemporal, and the matching x with them, through a ring of D chunks in registers
//              (D = 4 / 3 / 2 for MT = 1 / 2 / 4; the 64 x 64 tile keeps only its codes there): while a chunk is computed the
//              wavefront's next D - 1 are in flight.  Lane (col, g = l >> 4) holds, of weight row col, words 4 g .. 4 g + 3 of a
//              128-chunk (k = 32 g .. 32 g + 31) or word g of a 32-chunk; MFMA step j of the chunk takes word j.  The position
//              of a k inside a step is free as long as A and B agree, so the A fragment of step j is
//              x[row col][chunk + 32 g + 8 j ..  + 7]: the lane's matching 64 contiguous bytes of x as four plain cached
//              16-byte loads (x is re-read by every workgroup and lives in L2).  A B fragment is reused by the MT tiles of
//              x, an A fragment by the NT tiles of W.
//   decode     one 256-entry table per output row (alpha_per_row) or one per tensor, built once per workgroup:
//              the 4-bit byte table's one definition (antq_k_linear4.h: lin4_book, Lin4Entry), s = alpha / gmax.
//   sum        fp32 in the MFMA accumulator, a wavefront's chunks chained in rising order; the eight wavefronts' partial
//              tiles meet in LDS (the tables' memory, after a barrier) and are combined as
//              ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)), then the bias in fp32 and ONE rounding to the output type.
//              The sequence of operations that makes y[m, n] depends on K and the code path only -- not on M, N, MT, NT or
//              the other rows of x.
//   edges      rows m >= M, rows n >= N and lanes past the end of K clamp their addresses into the buffers; the x fragment
//              of such a row or lane is all zeros (it adds exactly +0), padded outputs are not stored.
// No atomics, no split of K across workgroups, no workspace: one launch, stream-ordered, capturable.
#ifndef ANTQ_K_LINEAR4_MM_H
#define ANTQ_K_LINEAR4_MM_H

#include "antq_k_linear4.h"

namespace antq {

constexpr int kMmWaves = 8;                            // wavefronts per workgroup = ways K is split
constexpr int mm_mtiles(size_t M) { return M <= 16 ? 1 : (M <= 32 ? 2 : 4); }   // 33 .. 48 rows run as 64

// NT, tiles of 16 output rows per workgroup.  A workgroup reads 8 NT K bytes of codes and re-reads M K 2 bytes of x from L2,
// so more rows of x want more rows of W per workgroup; fewer rows per workgroup mean more workgroups.  From the rows of
// profiles/packed_linear_mm.md "B with the tile rule overridden": below N = 8192 (N / 16 <= 256 workgroups at NT = 1) one tile was
// fastest in every row measured; at N = 16384 four tiles were fastest at M = 32 and 64 (by 1.3x and 1.6x over two), while at
// M = 8 four were 6-7 % faster than two and at M = 16 3-4 % slower -- one choice, two, is kept for M <= 16.
// N = 8192 was not measured.  The rule is the launcher's: no sum depends on it.
static inline int mm_ntiles(size_t M, size_t N)
{
    const int by_m = M <= 16 ? 2 : 4;
    const int by_n = N >= 4 * 4096 ? 4 : (N >= 2 * 4096 ? 2 : 1);
    return by_m < by_n ? by_m : by_n;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <typename T> struct MmOp;
template <> struct MmOp<bf16_tag> {
    typedef __bf16 frag_t __attribute__((ext_vector_type(8)));
    __device__ __forceinline__ static f32x4_t mfma(const u32x4_t &a, const u32x4_t &b, const f32x4_t &c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(frag_t, a), __builtin_bit_cast(frag_t, b), c, 0, 0, 0);
    }
};
template <> struct MmOp<f16_tag> {
    typedef _Float16 frag_t __attribute__((ext_vector_type(8)));
    __device__ __forceinline__ static f32x4_t mfma(const u32x4_t &a, const u32x4_t &b, const f32x4_t &c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(frag_t, a), __builtin_bit_cast(frag_t, b), c, 0, 0, 0);
    }
};

// MT: tiles of 16 rows of x; NT: tiles of 16 rows of W per workgroup; VEC: 16 B of codes per lane (K % 32 == 0, aligned)
template <typename T, bool OVP, int MT, int NT, bool VEC>
__global__ void __launch_bounds__(64 * kMmWaves)
k_linear4_mm(const uint32_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
             uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
             const float *__restrict__ grid, uint32_t m, int n_normal)
{
    constexpr int W = VEC ? 4 : 1;                     // code words per lane and chunk = MFMA steps per chunk
    constexpr int ROWS = 16 * NT;
    constexpr int TILES = MT * NT;
    constexpr int TAB_WORDS = ROWS * 256;             // (>= 2 tiles of 8 partial sums: the reduction's rounds fit in it)
    static_assert(kMmWaves == 8 && TAB_WORDS >= kMmWaves * 256, "the reduction below");
    __shared__ __attribute__((aligned(16))) uint32_t smem[TAB_WORDS];
    __shared__ float g[32];
    __shared__ float sc[ROWS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t row0 = blockIdx.x * (uint32_t)ROWS;
    const uint32_t wpr = K >> 3;                       // code words per row
    const uint32_t upr = wpr / W;                      // a lane's load units per row (VEC: K % 32 == 0)
    const uint32_t nchunks = (upr + 3u) >> 2;

    const ANTQ_GLOBAL uint32_t *crow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) crow[nt] = (const ANTQ_GLOBAL uint32_t *)(codes) + (size_t)min(row0 + 16u * nt + col, N - 1u) * wpr;
    const char *xrow[MT];
    bool mok[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        mok[mt] = 16u * mt + col < M;
        xrow[mt] = static_cast<const char *>(x) + (size_t)min(16u * mt + col, M - 1u) * K * 2u;
    }
    // a ring of D chunks in registers: while one is computed the wavefront's next D - 1 are in flight
    constexpr int D = MT == 1 ? 4 : (MT == 2 ? 3 : 2);
    constexpr bool XR = !(MT == 4 && NT == 4 && VEC);  // x rides in the ring too (the largest tile has no registers for it)
    uint32_t cw[D][NT][W];
    u32x4_t xa[XR ? D : 1][MT][W];
    auto load_x = [&](uint32_t c, u32x4_t (&xs)[MT][W]) {
        const uint32_t u0 = c * 4u + kg;
        const bool kok = u0 < upr;
        const size_t xoff = (size_t)min(u0, upr - 1u) * (16u * W); // bytes: a unit is 8 W elements of 2 bytes
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int j = 0; j < W; j++) {
                u32x4_t v = *(const ANTQ_GLOBAL u32x4_t *)(xrow[mt] + xoff + 16u * j);
                if (!(kok && mok[mt])) v = u32x4_t{0u, 0u, 0u, 0u};
                xs[mt][j] = v;
            }
    };
    auto load_chunk = [&](uint32_t c, int d) {
        const uint32_t u = min(c * 4u + kg, upr - 1u);             // (lanes past the row's end repeat its last unit; their x is 0)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            if constexpr (VEC) {
                const u32x4_t v = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(crow[nt]) + u);
                cw[d][nt][0] = v.x; cw[d][nt][1] = v.y; cw[d][nt][2] = v.z; cw[d][nt][3] = v.w;
            } else cw[d][nt][0] = __builtin_nontemporal_load(crow[nt] + u);
        }
        if constexpr (XR) load_x(c, xa[d]);
    };
#pragma unroll
    for (int d = 0; d < D; d++)                          // in flight while the tables are built
        if (wave + kMmWaves * d < nchunks) load_chunk(wave + kMmWaves * d, d);

    lin4_book(g, tid, grid, m);
    if (tid < (per_row ? (uint32_t)ROWS : 1u)) sc[tid] = ld_global(alpha + (per_row ? min(row0 + tid, N - 1u) : 0u)) / gmax;   // AQ:536 scale = alpha / max(grid)
    __syncthreads();
    {
        const uint32_t b = tid & 255u;                 // threads b and 256 + b make entry b of the even and the odd tables
        const Lin4Entry<T, OVP> e(b, g, n_normal);
        for (uint32_t r = tid >> 8; r < (per_row ? (uint32_t)ROWS : 1u); r += 2u) smem[r * 256u + b] = e.at(sc[r]);
    }
    __syncthreads();

    const uint32_t *tab[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) tab[nt] = smem + (per_row ? (16u * nt + col) * 256u : 0u);
    f32x4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

    for (uint32_t c0 = wave; c0 < nchunks; c0 += kMmWaves * D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t c = c0 + kMmWaves * d;
            if (c >= nchunks) break;
            if constexpr (!XR) load_x(c, xa[0]);
            const auto &xc = xa[XR ? d : 0];
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int j = 0; j < W; j++) {
                    const uint32_t word = cw[d][nt][j];
                    const u32x4_t b = {tab[nt][word & 0xffu], tab[nt][(word >> 8) & 0xffu], tab[nt][(word >> 16) & 0xffu], tab[nt][word >> 24]};
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[mt][nt] = MmOp<T>::mfma(xc[mt][j], b, acc[mt][nt]);
                }
            if (c + kMmWaves * D < nchunks) load_chunk(c + kMmWaves * D, d);
        }
    }

    // The eight partial tiles meet in LDS (the tables' memory, once every wavefront is done with them), G tiles per round:
    // red[slot][wave][reg][lane].  C / D map: column (n) = lane & 15, row (m) = 4 (lane >> 4) + reg.
    constexpr int G = TAB_WORDS / (kMmWaves * 256) < TILES ? TAB_WORDS / (kMmWaves * 256) : TILES;
    float *red = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int t0 = 0; t0 < TILES; t0 += G) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < G; s++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[((s * kMmWaves + wave) * 4 + r) * 64 + lane] = acc[(t0 + s) / NT][(t0 + s) % NT][r];
        __syncthreads();
        for (uint32_t s = wave; s < (uint32_t)G; s += kMmWaves) {             // slot s is finished by wavefront s % 8
            const uint32_t t = t0 + s, mt = t / NT, nt = t % NT;
            const uint32_t n = row0 + 16u * nt + col;
            const float bv = (bias && n < N) ? IO<T>::load1(bias, n) : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *p = red + (s * kMmWaves * 4u + r) * 64u + lane;       // wavefront w's partial sum: p[256 w]
                float v = ((p[0] + p[256]) + (p[512] + p[768])) + ((p[1024] + p[1280]) + (p[1536] + p[1792]));
                const uint32_t mrow = 16u * mt + 4u * kg + r;
                if (n < N && mrow < M) {
                    if (bias) v += bv;
                    IO<T>::store1(y, (size_t)mrow * N + n, v);
                }
            }
        }
    }
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR4_MM_H
