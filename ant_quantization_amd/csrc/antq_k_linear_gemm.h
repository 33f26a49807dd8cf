// antq_k_linear_gemm.h -- y = x . W^T (+ bias) for 1 .. 4096 rows of x on the matrix cores, straight from the packed codes of W:
// the kernel of antq_linear4_gemm and antq_linear8_gemm (bf16 and f16), written once over the codec (antq_k_linear4.h: Lin4Codec,
// antq_k_linear8.h: Lin8Codec).  Beyond 64 rows there are enough (M, N) tiles to fill the chip without
// splitting K, x is the operand worth staging through LDS, and the decode of a W element is amortised over every row of x a
// wavefront holds -- the shape antq_k_linear_mm.h (K split over eight wavefronts, x re-read from L2 in fragment-shaped loads)
// was not built for.
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
//   ownership  a workgroup of WAVES = 2 / 4 wavefronts owns one tile of BM = 64 WAVES rows of x by BN = 64 output rows n
//              (grid: x = tiles of n, y = tiles of m).  Wavefront w owns rows 64 w .. 64 w + 63 of the tile for all 64 n:
//              4 x 4 accumulator tiles of v_mfma_f32_16x16x32_{bf16,f16}.  A wavefront whose 64 rows lie past M only helps
//              to stage.  WAVES is the launcher's choice from M and N (gemm_waves; antq_debug_set key 23 forces it); no sum depends on it.
//   W          the decoder's own tables, one per output row (alpha_per_row) or one per tensor, laid out as the codec's MmLds
//              and read by its mm_b, so that W[n, k] is the element antq_decode4 / antq_decode8 writes: no widening, no scale
//              factored out.  4-bit: byte tables (Lin4Entry over dec4_book, i.e. dec_pair / DecOut; 64 KB), one 32-bit code
//              word is the 8 consecutive k of one weight row that a lane of the MFMA holds, four ds_read_b32 ARE the four
//              operand registers.  Bytes: the finished 16-bit outputs Dec8Out<T>::make(g * s) keyed by the code byte, with the
//              pair rule a second table for the outlier list (32 / 64 KB); two code words are a lane's 8 k, eight ds_read_u16
//              at dec8_slot(c, c of the byte next door) make the four registers.  The tables are built by the workgroup's own
//              wavefront count (bytes: Lin8Codec::gemm_build, rows w, w + WAVES, ...), the values bit for bit mm_build's.
//              A B fragment is made once per wavefront and step and reused over the wavefront's four row tiles of x.
//   codes      straight to registers, one step (BK = 128 elements of K) ahead of the MFMAs: 16 bytes (4-bit) or 32 bytes
//              (bytes) per lane, n-tile and step.  Lane (col, kg = lane >> 4) of n-tile nt holds, of weight row 16 nt + col,
//              VEC (16-byte loads; 4-bit: K % 32 == 0, bytes: K % 16 == 0; codes 16-byte aligned): the 32 elements
//              128 c + 32 kg .. + 31 of step c -- 4-bit the one load unit 4 c + kg, bytes the two units 2 (4 c + kg) and
//              + 1 (with K % 32 == 16 the second unit of the row's last lane group lies past the row's end: it repeats
//              the last unit and counts as k >= K) -- else (the codec's narrow load: 4 bytes / 8 bytes, K % 8 == 0): the
//              four groups of 8 elements 16 c + 4 j + kg, j = 0 .. 3.  MFMA j of the step takes the lane's words
//              WORDS j .. WORDS j + WORDS - 1, so the k a lane feeds to MFMA j is, for both widths,
//              128 c + 32 kg + 8 j .. + 7 (VEC) or 128 c + 32 j + 8 kg .. + 7: the piece of x that meets it is a function
//              of (kg, j) alone.
//   x          through LDS in full lines: per step the workgroup reads BM rows x 256 bytes (16 consecutive lanes one row's two
//              128-byte lines) into registers one step ahead and writes them as 16-byte pieces to a [BM][16] image whose
//              piece index is XORed with row & 15, so that the 16 rows of an A fragment (ds_read_b128 of piece 4 kg + j, VEC,
//              or 4 j + kg) fall on 16 different slots of the bank row.  One image, two barriers per step (image free /
//              image written); the global loads of step c + 1 are in flight while step c is computed.
//   sum        y[m, n] is ONE fp32 MFMA accumulator chain: steps c in rising order, MFMAs j = 0 .. 3 in rising order inside
//              a step, then the bias in fp32 and ONE rounding to the output type.  K is split neither across wavefronts nor
//              across workgroups.  The bits of y[m, n] depend on row m of x, row n of W, bias[n], K and the code path (VEC
//              or not) only -- not on M, N, WAVES, the other rows or the run.  The order is this kernel's own: it is neither
//              antq_linear4's / antq_linear8's (fp32 FMAs, e = 0 .. 7 per group) nor antq_linear4_mm's / antq_linear8_mm's
//              (eight partial chains and a fixed tree), so the same row of x has different low bits from the three.
//   edges      rows m >= M, rows n >= N and pieces with k >= K clamp their addresses into the buffers; the x of such a row or
//              piece is written to LDS as exactly zero, and the W fragment of a lane with k >= K is zero too (the last step,
//              one copy of the step after the loop; the index of the row's last group of 8 elements decides): padding adds
//              exactly +0 whatever the weights, Inf and NaN included.  Padded outputs are not stored.
// No atomics, no workspace: one launch, stream-ordered, capturable.  LDS: the x image (32 / 64 KB) and the tables -- 128 KB at
// the most for either width, of the CU's 160 KB.
// Measured, 4-bit (profiles/packed_linear4_gemm.md): 356 ... 404 TFLOP/s at best, slower than antq_decode4 + F.linear at every
// point (0.20 ... 0.92 of its speed).  Per step a wavefront issues 64 scattered ds_read_b32 look-ups beside 16 ds_read_b128 and 16
// ds_write_b128, the four wavefronts decode the same 64 output rows, and one wavefront per SIMD overlaps nothing with the two
// barriers: LDS- and latency-bound by that count (no hardware counters).  The byte form makes 128 look-ups per step, twice as
// many (profiles/packed_linear8_gemm.md).  The kernel buys memory and a free scratch, not speed.
#ifndef ANTQ_K_LINEAR_GEMM_H
#define ANTQ_K_LINEAR_GEMM_H

#include "antq_k_linear4.h"
#include "antq_k_linear8.h"

namespace antq {

constexpr int kGemmBN = 64;                            // output rows per workgroup
constexpr int kGemmBK = 128;                           // elements of K per staged step
constexpr int kGemmWaveRows = 64;                      // rows of x per wavefront; BM = 64 WAVES

// WAVES, wavefronts (tiles of 64 rows of x) per workgroup.  One workgroup runs per CU (LDS), and its time hardly depends on
// WAVES (profiles/packed_linear4_gemm.md, columns B128 / B256: 73 against 91 us per round of K = 4096), so the smaller tile
// is faster exactly while all of its workgroups run at once: 2 (BM = 128) while the tiles of 128 rows number at most the
// MI355X's 256 CUs -- the rule matched the faster forced shape at every point measured -- and 4 (BM = 256) beyond.  The rule
// is the launcher's: no sum depends on it.
constexpr size_t kGemmCUs = 256;
static inline int gemm_waves(size_t M, size_t N)
{
    return ((N + kGemmBN - 1) / kGemmBN) * ((M + 2 * kGemmWaveRows - 1) / (2 * kGemmWaveRows)) <= kGemmCUs ? 2 : 4;
}

// C: the codec (antq_k_linear4.h: Lin4Codec, antq_k_linear8.h: Lin8Codec).  Beside what antq_k_linear_mm.h names (Out, WORDS,
// Narrow, TS, MmEnt, MmLds<ROWS>, mm_b) it brings
//     gemm_build<ROWS, NW>(lds, ...)   (bytes) builds the tables of ROWS output rows with a workgroup of NW wavefronts, the
//                                      values bit for bit mm_build's; it ends WITHOUT a barrier (the first step's orders the
//                                      tables too).  The 4-bit build stands in the kernel (below).
//     PAIR                             (4-bit) the pair rule, for that build
// WAVES: wavefronts per workgroup; VEC: 16-byte loads of codes (K a multiple of the 16 bytes' elements, codes aligned)
template <typename C, int WAVES, bool VEC>
__global__ void __launch_bounds__(64 * WAVES)
k_linear_gemm(const uint32_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
              uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
              const float *__restrict__ grid, uint32_t m, int n_normal)
{
    typedef typename C::Out T;
    typedef typename C::MmEnt Ent;
    constexpr int W = C::WORDS;                        // code words of 8 elements: what one MFMA takes of a lane
    constexpr int MT = kGemmWaveRows / 16, NT = kGemmBN / 16;   // a wavefront's tiles of 16 rows of x, of 16 output rows
    constexpr int BM = kGemmWaveRows * WAVES, NTH = 64 * WAVES;
    constexpr int USH = W == 1 ? 5 : 4;                // (VEC) a row has K >> USH 16-byte load units
    constexpr int PIECES = kGemmBK / 8;                // 16-byte pieces of a row of x per step
    constexpr int XL = BM * PIECES / NTH;              // pieces a thread stages per step
    constexpr int RSTEP = NTH / PIECES;                // rows between a thread's pieces
    static_assert(PIECES == 16 && XL == 16 && kGemmBK == 32 * 4 && (W == 1 || W == 2), "the maps below");
    struct Lds {
        typename C::template MmLds<kGemmBN> w;         // the tables of 64 output rows (and what their build stages)
        u32x4_t xs[BM * PIECES];                       // the staged x: piece p of row r at [16 r + (p ^ (r & 15))]
    };
    __shared__ Lds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t n0 = blockIdx.x * (uint32_t)kGemmBN, m0 = blockIdx.y * (uint32_t)BM;
    const uint32_t wpr = (K >> 3) * (uint32_t)W;       // code words per row
    const uint32_t gpr = wpr / (uint32_t)W;            // groups of 8 elements per row (4-bit: the very value wpr, as that kernel was written)
    const uint32_t nsteps = (K + (uint32_t)kGemmBK - 1u) / (uint32_t)kGemmBK;
    const bool active = m0 + (uint32_t)kGemmWaveRows * wave < M;      // (wave-uniform) this wavefront has rows of x

    const ANTQ_GLOBAL uint32_t *crow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) crow[nt] = (const ANTQ_GLOBAL uint32_t *)(codes) + (size_t)min(n0 + 16u * nt + col, N - 1u) * wpr;

    // this thread's pieces of a step: piece tid & 15 of rows (tid >> 4) + RSTEP i
    const uint32_t xp = tid & 15u, xr0 = tid >> 4;
    u32x4_t xn[XL];
    uint32_t cwn[NT][4 * W];                           // MFMA j of the step takes words W j ... W j + W - 1
    auto load_step = [&](uint32_t c) {
        const uint32_t k0 = c * (uint32_t)kGemmBK + 8u * xp;
        const bool kok = k0 < K;
        const size_t koff = (size_t)min(k0, K - 8u) * 2u;
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t r = m0 + xr0 + (uint32_t)(RSTEP * i);
            u32x4_t v = *(const ANTQ_GLOBAL u32x4_t *)(static_cast<const char *>(x) + (size_t)min(r, M - 1u) * K * 2u + koff);
            if (!(kok && r < M)) v = u32x4_t{0u, 0u, 0u, 0u};
            xn[i] = v;
        }
        if (active) {
            if constexpr (VEC) {
                uint32_t u[W];                         // (units past the row's end repeat its last; their x and their B are 0)
#pragma unroll
                for (int l = 0; l < W; l++) u[l] = min((c * 4u + kg) * (uint32_t)W + (uint32_t)l, (K >> USH) - 1u);
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
#pragma unroll
                    for (int l = 0; l < W; l++) {
                        uint32_t t[4];
                        lin_words(*((const ANTQ_GLOBAL u32x4_t *)(crow[nt]) + u[l]), t);
#pragma unroll
                        for (int i = 0; i < 4; i++) cwn[nt][4 * l + i] = t[i];
                    }
            } else {
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if constexpr (W == 1) {
                            cwn[nt][j] = crow[nt][min(c * 16u + 4u * j + kg, gpr - 1u)];
                        } else {
                            const uint32_t g8 = min(c * 16u + 4u * j + kg, gpr - 1u);
                            const u32x2_t v = *((const ANTQ_GLOBAL u32x2_t *)(crow[nt]) + g8);
                            cwn[nt][2 * j] = v.x;
                            cwn[nt][2 * j + 1] = v.y;
                        }
                    }
            }
        }
    };
    load_step(0u);                                     // in flight while the tables are built

    // The tables, the values bit for bit mm_build's; no barrier after them (the first step's orders them before the reads).
    if constexpr (W == 1) {
        // 4-bit: entry b of row r is Lin4Entry(b).at(alpha[r] / gmax).  These lines stay HERE and not behind a call into the
        // codec: from there the compiler schedules this prologue differently, and the 4-bit variants keep the
        // instruction sequence they were measured with.
        dec4_book(lds.w.g, tid, grid, m);
        if (tid < (per_row ? (uint32_t)kGemmBN : 1u)) lds.w.sc[tid] = ld_global(alpha + (per_row ? min(n0 + tid, N - 1u) : 0u)) / gmax;   // AQ:536 scale = alpha / max(grid)
        __syncthreads();
        for (uint32_t b = tid; b < 256u; b += (uint32_t)NTH) {
            const Lin4Entry<T, C::PAIR> e(b, lds.w.g, n_normal);
            for (uint32_t r = 0; r < (per_row ? (uint32_t)kGemmBN : 1u); r++) lds.w.tab[r * 256u + b] = e.at(lds.w.sc[r]);
        }
    } else {
        C::template gemm_build<kGemmBN, WAVES>(lds.w, tid, n0, N, alpha, per_row, gmax, grid, m, n_normal);
    }

    const Ent *tab[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) tab[nt] = lds.w.tab + (per_row ? (16u * nt + col) * C::TS : 0u);
    f32x4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

    uint32_t cw[NT][4 * W];
    // One step.  Only the last step can hold pieces with k >= K: the loop leaves it to ONE copy of the step after it (TAIL),
    // in which the B fragment of a lane with k >= K is zero like its x -- 0 * W is +0 only for a finite W, and the lane repeats
    // the row's last unit, whatever that holds.
    const uint32_t nmain = (K % (uint32_t)kGemmBK) ? nsteps - 1u : nsteps;
    auto step = [&](uint32_t c, auto TAIL) {
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t r = xr0 + (uint32_t)(RSTEP * i);
            lds.xs[r * PIECES + (xp ^ (r & 15u))] = xn[i];
        }
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int j = 0; j < 4 * W; j++) cw[nt][j] = cwn[nt][j];
        __syncthreads();                               // the image (and, the first time, the tables) written
        if constexpr (!decltype(TAIL)::value)
            if (c + 1u < nsteps) load_step(c + 1u);
        if (active) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                u32x4_t b[NT];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) b[nt] = C::mm_b(tab[nt], &cw[nt][W * j]);
                if constexpr (decltype(TAIL)::value) {
                    // (the group of 8 elements MFMA j takes of this lane lies inside the row: VEC by its 16-byte unit)
                    const bool kok = VEC ? (c * 4u + kg) * (uint32_t)W + (uint32_t)(W * j / 4) < (K >> USH) : c * 16u + 4u * j + kg < gpr;
#pragma unroll
                    for (int nt = 0; nt < NT; nt++)
                        if (!kok) b[nt] = u32x4_t{0u, 0u, 0u, 0u};
                }
                const uint32_t p = VEC ? 4u * kg + j : 4u * j + kg;
#pragma unroll
                for (int mt = 0; mt < MT; mt++) {
                    const u32x4_t a = lds.xs[((uint32_t)kGemmWaveRows * wave + 16u * mt + col) * PIECES + (p ^ col)];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) acc[mt][nt] = MmOp<T>::mfma(a, b[nt], acc[mt][nt]);
                }
            }
        }
    };
    for (uint32_t c = 0; c < nmain; c++) {
        step(c, std::false_type{});
        __syncthreads();                               // the image free again
    }
    if (nmain < nsteps) step(nmain, std::true_type{});

    // C / D map: column (n) = lane & 15, row (m) = 4 (lane >> 4) + reg
    if (!active) return;
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const uint32_t n = n0 + 16u * nt + col;
        if (n >= N) continue;
        const float bv = bias ? IO<T>::load1(bias, n) : 0.0f;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + (uint32_t)kGemmWaveRows * wave + 16u * mt + 4u * kg + r;
                if (mrow < M) {
                    float v = acc[mt][nt][r];
                    if (bias) v += bv;
                    IO<T>::store1(y, (size_t)mrow * N + n, v);
                }
            }
    }
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR_GEMM_H
