// antq_k_linear8_mm.h -- y = x . W^T (+ bias) for 1 .. 64 rows of x on the matrix cores, straight from the BYTE codes of W
// (antq_linear8_mm; bf16 and f16).  Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// The byte-code twin of antq_k_linear4_mm.h (MmOp, mm_mtiles, mm_ntiles, kMmWaves and f32x4_t are that header's): the same
// ownership, ring, sum and edges, with the byte decoder's rule (antq_k_decbatch8.h: dec8_book, dec8_slot, Dec8Out) for the
// weights, so that W[n, k] IS the element antq_decode8 writes.  The B fragment of lane l for one step of
// v_mfma_f32_16x16x32_{bf16,f16} is 8 consecutive k of ONE weight row (col = l & 15, kg = l >> 4): 8 bytes, two code words.  An
// element's partner under the pair rule (flat pairs (2k, 2k + 1)) is the neighbouring byte of the same word: nothing
// crosses a lane.
//
//   ownership  workgroups of 8 wavefronts; a workgroup owns 16 NT consecutive output rows n for all MT tiles of 16 rows of
//              x.  K is cut into chunks of 64 elements (VEC: 16 B of codes per lane, two MFMA steps) or 32 (8 B per lane, one
//              step); wavefront w takes chunks w, w + 8, w + 16, ... in rising order: a function of K and the code path alone.
//   loads      codes straight to VGPRs, nontemporal, and the matching x (plain cached 16-byte loads) with them, through a
//              ring of D chunks in registers (D = 4 / 3 / 2 for MT = 1 / 2 / 4).  Lane (col, kg) holds, of weight row col,
//              bytes 16 u .. 16 u + 15 (VEC) or 8 u .. 8 u + 7 of the row, u = 4 chunk + kg; step j takes words 2 j, 2 j + 1, and
//              the A fragment of step j is the same 8 elements of x: A and B agree on the k of every position.
//   decode     one table per output row (alpha_per_row) or one per tensor, built once per workgroup, of the decoder's own
//              finished 16-bit outputs keyed by the code byte -- Dec8Out<T>::make(g * s), g from dec8_book (with its + 0.0f),
//              s = alpha / gmax, the multiplication done for every entry as the decoder does it -- and with the pair rule a
//              second one of 256 entries for the outlier list; entry 255 of both is +0.  An element is one 16-bit LDS read
//              at dec8_slot(c, c_partner); two of them are one operand register.  Every wavefront holds the book in
//              registers (dec8_book's four entries per lane) and builds whole rows r = w, w + 8, ...: no staging array and
//              no second barrier.  16 NT rows x 256 or 512 entries x 2 B: 64 KB at the most (NT = 4, pair rule), and
//              nothing else lives in LDS, so no variant needs more than the 64 KB every launch may have.
//   sum        fp32 in the MFMA accumulator, a wavefront's chunks chained in rising order; the eight partial tiles meet in
//              LDS (the tables' memory, after a barrier; 8 KB per tile and round) and are combined as
//              ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)), then the bias in fp32 and ONE rounding to the output type.
//              y[m, n] depends on K and the code path only -- not on M, N, MT, NT or the other rows of x.
//   edges      rows m >= M, rows n >= N and lanes past the end of K clamp their addresses into the buffers; the x fragment
//              of such a row or lane is all zeros (it adds exactly +0), padded outputs are not stored.
// No atomics, no split of K across workgroups, no workspace: one launch, stream-ordered, capturable.
#ifndef ANTQ_K_LINEAR8_MM_H
#define ANTQ_K_LINEAR8_MM_H

#include "antq_k_decbatch8.h"
#include "antq_k_linear4_mm.h"

namespace antq {

// MT: tiles of 16 rows of x; NT: tiles of 16 rows of W per workgroup; VEC: 16 B of codes per lane (K % 16 == 0, aligned)
template <typename T, bool OVP, int MT, int NT, bool VEC>
__global__ void __launch_bounds__(64 * kMmWaves)
k_linear8_mm(const uint32_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
             uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
             const float *__restrict__ grid, uint32_t m, int n_normal)
{
    typedef typename Dec8Out<T>::Ent Ent;              // (16 bits)
    typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
    constexpr int S = VEC ? 2 : 1;                     // MFMA steps per chunk; a step is two code words per lane
    constexpr int ROWS = 16 * NT;
    constexpr int TILES = MT * NT;
    constexpr uint32_t TS = OVP ? 512u : 256u;         // entries of one row's table(s)
    constexpr int TAB_WORDS = ROWS * (int)TS / 2;      // (>= one tile of 8 partial sums: the reduction's rounds fit in it)
    static_assert(sizeof(Ent) == 2 && kMmWaves == 8 && TAB_WORDS >= kMmWaves * 256 && TAB_WORDS * 4 <= 65536, "the tables and the reduction below");
    __shared__ __attribute__((aligned(16))) uint32_t smem[TAB_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t row0 = blockIdx.x * (uint32_t)ROWS;
    const uint32_t wpr = K >> 2;                       // code words per row
    const uint32_t upr = (K >> 3) / S;                 // a lane's load units per row (VEC: K % 16 == 0)
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
    uint32_t cw[D][NT][2 * S];
    u32x4_t xa[D][MT][S];
    auto load_chunk = [&](uint32_t c, int d) {
        const uint32_t u0 = c * 4u + kg;
        const bool kok = u0 < upr;
        const uint32_t u = min(u0, upr - 1u);                      // (lanes past the row's end repeat its last unit; their x is 0)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            if constexpr (VEC) {
                const u32x4_t v = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(crow[nt]) + u);
                cw[d][nt][0] = v.x; cw[d][nt][1] = v.y; cw[d][nt][2] = v.z; cw[d][nt][3] = v.w;
            } else {
                const u32x2_t v = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x2_t *)(crow[nt]) + u);
                cw[d][nt][0] = v.x; cw[d][nt][1] = v.y;
            }
        }
        const size_t xoff = (size_t)u * (16u * S);                 // bytes: a unit is 8 S elements of 2 bytes
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int j = 0; j < S; j++) {
                u32x4_t v = *(const ANTQ_GLOBAL u32x4_t *)(xrow[mt] + xoff + 16u * j);
                if (!(kok && mok[mt])) v = u32x4_t{0u, 0u, 0u, 0u};
                xa[d][mt][j] = v;
            }
    };
#pragma unroll
    for (int d = 0; d < D; d++)                          // in flight while the tables are built
        if (wave + kMmWaves * d < nchunks) load_chunk(wave + kMmWaves * d, d);

    Ent *tab16 = reinterpret_cast<Ent *>(smem);
    {
        // the decoder's own table (dec8_row_task): this lane's four entries of the book, every row's scale applied to them
        DecDesc B;
        B.grid = grid; B.m = m; B.n_normal = n_normal;
        float nv[4], ov[4];
        dec8_book<OVP>(B, lane, nv, ov);
        for (uint32_t r = wave; r < (per_row ? (uint32_t)ROWS : 1u); r += kMmWaves) {
            const float s = ld_global(alpha + (per_row ? min(row0 + r, N - 1u) : 0u)) / gmax;   // AQ:536 scale = alpha / max(grid)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t b = lane + 64u * k;
                tab16[r * TS + b] = Dec8Out<T>::make(nv[k] * s);
                if (OVP) tab16[r * TS + 256u + b] = Dec8Out<T>::make(ov[k] * s);
            }
        }
    }
    __syncthreads();

    const Ent *tab[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) tab[nt] = tab16 + (per_row ? (16u * nt + col) * TS : 0u);
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
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int j = 0; j < S; j++) {
                    uint32_t cb[8];
#pragma unroll
                    for (int e = 0; e < 4; e++) { cb[e] = (cw[d][nt][2 * j] >> (8 * e)) & 0xffu; cb[4 + e] = (cw[d][nt][2 * j + 1] >> (8 * e)) & 0xffu; }
                    uint32_t o[4];
#pragma unroll
                    for (int p = 0; p < 4; p++) {                   // (flat pairs (2k, 2k + 1): the partner is the byte next door)
                        const uint32_t lo = tab[nt][dec8_slot<OVP>(cb[2 * p], cb[2 * p + 1])], hi = tab[nt][dec8_slot<OVP>(cb[2 * p + 1], cb[2 * p])];
                        o[p] = lo | (hi << 16);
                    }
                    const u32x4_t b = {o[0], o[1], o[2], o[3]};
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[mt][nt] = MmOp<T>::mfma(xa[d][mt][j], b, acc[mt][nt]);
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

#endif  // ANTQ_K_LINEAR8_MM_H
