// antq_k_linear_mm.h -- y = x . W^T (+ bias) for 1 .. 64 rows of x on the matrix cores, straight from the packed codes of W: the
// kernel of antq_linear4_mm and antq_linear8_mm (bf16 and f16), written once.  A codec (antq_k_linear4.h: Lin4Codec,
// antq_k_linear8.h: Lin8Codec, the row-streaming kernel's) says how wide a code is, how the decoder's tables are built and how the
// B fragment of one MFMA step comes out of a lane's code words; everything else is here.
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// Beyond a handful of rows the arithmetic of a packed linear belongs on the matrix cores, and the layout of antq_encode4 /
// antq_encode8 fits v_mfma_f32_16x16x32_{bf16,f16}: the B fragment of lane l is B[k = 8 (l >> 4) + j][col l & 15], j = 0 .. 7 -- 8
// consecutive k of ONE weight row, which is one 32-bit code word (4-bit) or two (bytes).  The tables hold the decoder's own
// finished outputs in the output type, so W[n, k] IS the element antq_decode4 / antq_decode8 writes, with no widening and no
// multiply; under the pair rule an element's partner is in the same word: nothing crosses a lane.
//
//   ownership  workgroups of 8 wavefronts; a workgroup owns 16 NT consecutive output rows n (NT = 1 / 2 / 4, the launcher's
//              choice from M and N) for all MT = 1 / 2 / 4 tiles of 16 rows of x.  K is cut into chunks: a lane's load of codes
//              (VEC: 16 B, else the codec's narrow load of 8 elements) is S MFMA steps of 8 elements, a chunk is 32 S elements
//              -- 4-bit: 128 (VEC) or 32, bytes: 64 (VEC) or 32.  Wavefront w takes chunks w, w + 8, w + 16, ... in rising
//              order: the split is a function of K and of the code path alone.
//   loads      codes straight to VGPRs, nontemporal, and the matching x with them, through a ring of D chunks in registers
//              (D = 4 / 3 / 2 for MT = 1 / 2 / 4; where the codec says so -- the 4-bit 64 x 64 VEC tile -- the ring keeps only
//              the codes and x is loaded as its chunk is computed): while a chunk is computed the wavefront's next D - 1 are
//              in flight.  Lane (col, kg = l >> 4) holds, of weight row col, load unit u = 4 chunk + kg of the row; MFMA
//              step j of the chunk takes the unit's words WORDS j ...  The position of a k inside a step is free as long as A
//              and B agree, so the A fragment of step j is x[row col][8 (S u + j) ..  + 7]: the lane's matching 16 S
//              contiguous bytes of x as plain cached 16-byte loads (x is re-read by every workgroup and lives in L2).  A B
//              fragment is reused by the MT tiles of x, an A fragment by the NT tiles of W.
//   decode     one table per output row (alpha_per_row) or one per tensor, built once per workgroup with s = alpha / gmax:
//              the codec's (4-bit: 256 words keyed by the code byte, a pair's two outputs each, so four ds_read_b32 ARE the
//              four operand registers; bytes: 256 16-bit outputs, with the pair rule 256 more for the outlier list, an element
//              one read at dec8_slot(c, c_partner) and two of them one operand register)
//   sum        fp32 in the MFMA accumulator, a wavefront's chunks chained in rising order; the eight wavefronts' partial
//              tiles meet in LDS (the tables' memory, after a barrier; 8 KB per tile and round) and are combined as
//              ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)), then the bias in fp32 and ONE rounding to the output type.
//              Two contracts, for both codecs:
//              (1) The sequence of operations that makes y[m, n] depends on K and the code path only -- not on M, N, MT, NT
//                  or the other rows of x.
//              (2) The fixed tree over the eight wavefronts.
//   edges      rows m >= M, rows n >= N and lanes past the end of K clamp their addresses into the buffers; the x fragment
//              of such a row or lane is all zeros, and so is the W fragment of a lane past the end of K (the row's last
//              chunk, which runs after the ring in a step of its own): padding adds exactly +0 whatever the weights, Inf and
//              NaN included.  Padded outputs are not stored.
// No atomics, no split of K across workgroups, no workspace: one launch, stream-ordered, capturable.
#ifndef ANTQ_K_LINEAR_MM_H
#define ANTQ_K_LINEAR_MM_H

#include "antq_k_linear.h"

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

// C: the codec.  Beside Out, WORDS, Narrow, TS and row_bytes(K) (antq_k_linear.h) it names
//     MmEnt                        a table entry
//     MmLds<ROWS>                  the workgroup's LDS: `tab`, the tables of ROWS output rows (TS entries per row, 16-byte
//                                  aligned; the reduction reuses this memory), and what the build stages
//     mm_build<ROWS>(lds, ...)     builds the tables, all 512 threads; ends with the barrier that orders them before the reads
//     mm_x_in_ring(MT, NT, VEC)    whether x rides in the ring with the codes
//     mm_tail_in_ring(MT, NT, VEC) whether a row's partial last chunk stays in the ring (every chunk then pays a select on
//                                  its B fragments) or gets a step of its own after it (below)
//     mm_b(t, w)                   the B fragment of one MFMA step from the WORDS code words w (t = the row's table)
// MT: tiles of 16 rows of x; NT: tiles of 16 rows of W per workgroup; VEC: 16 B of codes per lane (K a multiple of the 16 bytes'
// elements, codes aligned)
template <typename C, int MT, int NT, bool VEC>
__global__ void __launch_bounds__(64 * kMmWaves)
k_linear_mm(const uint32_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
            uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
            const float *__restrict__ grid, uint32_t m, int n_normal)
{
    typedef typename C::Out T;
    typedef typename C::MmEnt Ent;
    typedef std::conditional_t<VEC, u32x4_t, typename C::Narrow> Load;
    constexpr int CW = sizeof(Load) / 4;               // code words per lane, row and chunk
    constexpr int S = CW / C::WORDS;                   // MFMA steps per chunk
    constexpr int ROWS = 16 * NT;
    constexpr int TILES = MT * NT;
    __shared__ typename C::template MmLds<ROWS> lds;
    constexpr int TAB_WORDS = sizeof(lds.tab) / 4;     // (>= one tile of 8 partial sums: the reduction's rounds fit in it)
    static_assert(kMmWaves == 8 && TAB_WORDS >= kMmWaves * 256, "the reduction below");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t row0 = blockIdx.x * (uint32_t)ROWS;
    const uint32_t wpr = (uint32_t)(C::row_bytes(K) >> 2);   // code words per row
    const uint32_t upr = (K >> 3) / S;                 // a lane's load units per row (VEC: K a multiple of 8 S)
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
    constexpr bool XR = C::mm_x_in_ring(MT, NT, VEC);
    uint32_t cw[D][NT][CW];
    u32x4_t xa[XR ? D : 1][MT][S];
    // load unit u = 4 c + kg of chunk c, clamped into the row (lanes past the row's end repeat its last unit; their x and their B are 0)
    auto unit = [&](uint32_t c, bool &kok) {
        const uint32_t u0 = c * 4u + kg;
        kok = u0 < upr;
        return min(u0, upr - 1u);
    };
    auto load_x = [&](uint32_t u, bool kok, u32x4_t (&xs)[MT][S]) {
        const size_t xoff = (size_t)u * (16u * S);                 // bytes: a unit is 8 S elements of 2 bytes
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int j = 0; j < S; j++) {
                u32x4_t v = *(const ANTQ_GLOBAL u32x4_t *)(xrow[mt] + xoff + 16u * j);
                if (!(kok && mok[mt])) v = u32x4_t{0u, 0u, 0u, 0u};
                xs[mt][j] = v;
            }
    };
    auto load_chunk = [&](uint32_t c, int d) {
        bool kok;
        const uint32_t u = unit(c, kok);
#pragma unroll
        for (int nt = 0; nt < NT; nt++) lin_words(__builtin_nontemporal_load((const ANTQ_GLOBAL Load *)(crow[nt]) + u), cw[d][nt]);
        if constexpr (XR) load_x(u, kok, xa[d]);
    };
    // The ring serves the row's full chunks.  A partial last chunk is the last chunk of wavefront `towner` and runs after the
    // ring, from slot 0 -- loaded here already when that wavefront has no full chunk before it: rows of at most 8 chunks, whose
    // chunks all go to slot 0 of a wavefront each.
    constexpr bool TIR = C::mm_tail_in_ring(MT, NT, VEC);
    const uint32_t nfull = TIR ? nchunks : upr >> 2;     // (TIR: the ring serves every chunk, and no wavefront owns a tail)
    const uint32_t towner = nfull < nchunks ? (nfull & (kMmWaves - 1u)) : ~0u;
    const bool tearly = nfull < kMmWaves;
    const uint32_t nfirst = tearly ? nchunks : nfull;
#pragma unroll
    for (int d = 0; d < D; d++)                          // in flight while the tables are built
        if (wave + kMmWaves * d < nfirst) load_chunk(wave + kMmWaves * d, d);

    C::template mm_build<ROWS>(lds, tid, row0, N, alpha, per_row, gmax, grid, m, n_normal);

    const Ent *tab[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) tab[nt] = lds.tab + (per_row ? (16u * nt + col) * C::TS : 0u);
    f32x4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

    for (uint32_t c0 = wave; c0 < nfull; c0 += kMmWaves * D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t c = c0 + kMmWaves * d;
            if (c >= nfull) break;
            if constexpr (!XR) {
                bool kok;
                const uint32_t u = unit(c, kok);
                load_x(u, kok, xa[0]);
            }
            const auto &xc = xa[XR ? d : 0];
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int j = 0; j < S; j++) {
                    u32x4_t b = C::mm_b(tab[nt], &cw[d][nt][C::WORDS * j]);
                    if constexpr (TIR)
                        if (c * 4u + kg >= upr) b = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[mt][nt] = MmOp<T>::mfma(xc[mt][j], b, acc[mt][nt]);
                }
            if (c + kMmWaves * D < nfull) load_chunk(c + kMmWaves * D, d);
        }
    }
    // The row's partial last chunk, the last of the wavefront it falls to, in ring slot 0.  The B fragment of a lane past the
    // row's end is zero like its x: 0 * W is +0 only for a finite W, and the lane holds the row's repeated last unit.
    if (!TIR && wave == towner) {
        uint32_t ct = nfull;
        // (an empty statement the compiler cannot see through: the chunk's addresses are made here and not kept through
        // the loop, 2 VGPRs less in the byte-code pair-rule variants -- profiles/packed_linear_specials.md)
        asm volatile("" : "+s"(ct));
        if (!tearly) load_chunk(ct, 0);
        bool kok;
        const uint32_t u = unit(ct, kok);
        if constexpr (!XR) load_x(u, kok, xa[0]);
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int j = 0; j < S; j++) {
                u32x4_t b = C::mm_b(tab[nt], &cw[0][nt][C::WORDS * j]);
                if (!kok) b = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
                for (int mt = 0; mt < MT; mt++) acc[mt][nt] = MmOp<T>::mfma(xa[0][mt][j], b, acc[mt][nt]);
            }
    }

    // The eight partial tiles meet in LDS (the tables' memory, once every wavefront is done with them), G tiles per round:
    // red[slot][wave][reg][lane].  C / D map: column (n) = lane & 15, row (m) = 4 (lane >> 4) + reg.
    constexpr int G = TAB_WORDS / (kMmWaves * 256) < TILES ? TAB_WORDS / (kMmWaves * 256) : TILES;
    float *red = reinterpret_cast<float *>(lds.tab);
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

#endif  // ANTQ_K_LINEAR_MM_H
