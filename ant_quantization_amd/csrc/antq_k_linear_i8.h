// antq_k_linear_i8.h -- y = (xq . V^T) * u_x * u_w (+ bias) in the INTEGER domain, straight from the packed 4-bit codes of W [N, K]:
// the kernel of antq_linear4_i8 (fp32, bf16 and f16 outputs).  xq is the int8 image of the activations (antq_quant_i8), V[n, k] the
// int8 image of the weight's code; the sum over k is an exact int32 sum on v_mfma_i32_16x16x64_i8, the scales are applied once per
// output.  This is NOT the image product of the other packed linears: the scale is factored out of the sum (include/antq.h).
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.  Everything below but the source of the
// A operand lives in i8_tile, which antq_k_conv_i8.h shares: k_linear_i8 is i8_tile with the matrix A side (I8Matrix).
//
//   ownership  a workgroup of WAVES = 2 / 4 wavefronts owns one tile of BM = 16 MT WAVES rows of xq by BN = 64 output rows n
//              (grid: x = tiles of n, y = tiles of m).  Wavefront w owns rows 16 MT w .. + 16 MT - 1 of the tile for all 64 n:
//              MT x 4 accumulator tiles of v_mfma_i32_16x16x64_i8, MT = 4 (64 rows per wavefront) except for the 64-row tile of
//              calls with M <= 64 (WAVES = 2, MT = 2).  A wavefront whose rows lie past M stages and decodes but runs no MFMA.
//              The shape is the launcher's choice (i8_shape; antq_debug_set key 23 forces WAVES); sums are exact, so no result
//              depends on it.  K is split neither across wavefronts nor across workgroups.
//   W          decoded ONCE per workgroup and stage of BK = 128 k, as k_linear_t_gemm does.  The 64 x 64 bytes of codes of a
//              stage are 256 pieces of 16 bytes: piece q = (n = q >> 2, qk = q & 3) holds the 32 consecutive k 32 qk .. + 31 of
//              output row n, and thread t owns the pieces t, t + 64 WAVES, ... (one at 4 wavefronts, two at 2).  Four
//              consecutive lanes read the 64 contiguous bytes of one row.  A piece's 32 nibbles become 32 int8 in eight
//              registers and go to LDS as two ds_write_b128: the operands of lane groups kg = 2 (qk & 1) and + 1 of MFMA step
//              j = qk >> 1.
//   decode     plain books (m <= 16): in registers.  The 16-byte image sits in four registers T0 .. T3 (img); per code word (8 k):
//              the even and the odd nibbles' low three bits are the selectors of two v_perm_b32 each (T1:T0 and T3:T2), a
//              third v_perm_b32 whose selector carries bit 3 picks between the two results per byte, and two more interleave
//              even and odd elements into k order -- 15 VALU instructions per 8 weights, no LDS look-up.  Pair-rule books: a
//              256-entry LDS table of int8 pairs keyed by the code byte, built once per workgroup from the image with the
//              decoder's pair rule (dec_pair: a victim is 0, its partner reads image[n_normal + c]); per code word four
//              ds_read_u16 and the merges.
//   B image    [step j][n tile nt][kg][16 slots of 16 bytes], slot = n-in-tile ^ (4 j + (kg & 2)).  The lanes (col, kg) of a
//              wavefront read the fragment of (j, nt) as 64 different slots of one 1 KiB block with one ds_read_b128 each, no
//              bank conflict; the XOR is for the writes, where 8 consecutive lanes hold 2 rows x 4 pieces: they land on the
//              8 different 16-byte bank groups.  Two images (2 x 8 KiB): stage c + 1 is decoded beside the MFMAs of stage c.
//   codes      a stage's loads are issued one stage before its decode: while stage c is computed and stage c + 1 decoded from
//              registers, the loads of stage c + 2 are in flight.
//   xq         through LDS in full 128-byte lines: per stage BM rows x 128 bytes (8 consecutive lanes one row), read into
//              registers one stage ahead, written as 16-byte pieces to a [BM][8] image.  The swizzle is this kernel's own, not
//              k_linear_gemm's (whose rows hold 16 pieces): piece p of row r sits at 8 r + (p ^ (r & 7)), so that the 8 rows
//              8 consecutive lanes of an A fragment's ds_read_b128 (piece 4 j + kg of rows 16 mt + col) read fall on the 8
//              different 16-byte bank groups; rows r and r + 8 share one, in different octets of lanes.  One image, two
//              barriers per stage.
//   sum        S[m, n] = sum_k xq[m, k] V[n, k] in the int32 MFMA accumulator: exact (the launcher refuses I_x I_w K >= 2^31),
//              so it has no order.  Epilogue in registers: fl32(S), * u_x, * u_w[n], + bias[n] -- each a separate fp32
//              operation rounded once (no contraction: -ffp-contract=off), u_x = alpha_x / I_x and u_w[n] = alpha_w[n] / I_w
//              true fp32 divisions -- then ONE conversion to the output type.  The bits of y[m, n] depend on row m of xq, row
//              n of the codes, the scales and the bias, on nothing else.
//   edges      K % 32 == 0, N arbitrary.  A piece of codes with n >= N or k >= K (the last stage only) loads nothing and is
//              written as zero; a piece of xq with m >= M or k >= K clamps its address and is staged as zero: padding adds
//              exact zeros on both operands.  Padded outputs are not stored.
//   store      through the fixed C / D map (column n = lane & 15, row m = 4 (lane >> 4) + reg): 16 consecutive elements per row.
// No atomics, no workspace: one launch, stream-ordered, capturable.  LDS (WAVES = 4): xq image 32 KiB, B images 16 KiB, pair
// table and image 1 KiB -- three workgroups would fit a CU's 160 KiB; the registers (about 100 VGPRs + 128 AGPRs) allow two.
// Measured (profiles/int_linear4.md): up to 1212 TOP/s at M = 4096; in float32 2 ... 8 times faster than F.linear on the image
// from 512 rows up, in bfloat16 slower than it nearly everywhere (1.1 ... 1.5 times its time at 4096 rows) and 1.6 ... 3.3 times
// faster than antq_linear4_gemm at 4096 rows; at up to 64 rows the time hardly depends on M and follows K (one workgroup walks
// all of K): slower than every alternative there.
#ifndef ANTQ_K_LINEAR_I8_H
#define ANTQ_K_LINEAR_I8_H

#include "antq_k_linear_gemm.h"

// (every fp32 operation of the epilogue stays a scalar VALU instruction: one rounding per written operation)
#if defined(__HIP_DEVICE_COMPILE__)
#define ANTQ_I8_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define ANTQ_I8_KERNEL
#endif

namespace antq {

typedef int i32x4_t __attribute__((ext_vector_type(4)));

// (WAVES, MT) of a call: the 64-row tile when M <= 64, else k_linear_gemm's rule between 128 and 256 rows -- the smaller tile
// while all of its workgroups run at once.  Sums are exact: the choice is for occupancy alone.
static inline void i8_shape(size_t M, size_t N, int forced_waves, int &waves, int &mt)
{
    if (M <= 64 && forced_waves == 0) { waves = 2; mt = 2; return; }
    waves = forced_waves ? forced_waves : gemm_waves(M, N);
    mt = 4;
}

// The slices of K of the split-K forms (antq_k_linear_i8_sk.h, M <= 64; antq_k_conv_i8_sk.h, row tiles of 64) on a part of
// `cus` compute units.  tiles = ceil(N / 64) ceil(M / 64) workgroups exist per slice, Mt = min(M, 64) rows per row tile, a
// slice is a whole number of 128-k stages:
//   S = the smallest of 1, 2, 4, 8, 16 with tiles S >= 2 cus (16 when none has)      two workgroups per CU
//   S <= K / (16 Mt)       per row tile: above it the 8 S Mt N bytes of partial traffic exceed the N K / 2 bytes of codes
//   S <= stages; forced (antq_debug_set key 24, 1 .. 16) replaces the rule and is clamped to stages alone
//   per_slice = ceil(stages / S) stages, and S becomes the number of non-empty slices, ceil(stages / per_slice)
// The sum is exact, so no result depends on S: the rule is for time alone.
static inline int i8_sk_slices(size_t M, size_t N, size_t K, int cus, int forced, size_t &per_slice)
{
    const size_t tiles = ((N + 63) / 64) * ((M + 63) / 64), stages = (K + 127) / 128;
    size_t S = 16;
    for (size_t s = 1; s <= 16; s *= 2)
        if (tiles * s >= 2 * (size_t)std::max(cus, 1)) { S = s; break; }
    S = std::min(S, std::max<size_t>(K / (16 * std::min<size_t>(M, 64)), 1));
    if (forced >= 1) S = (size_t)std::min(forced, 16);
    S = std::max<size_t>(std::min(S, stages), 1);
    per_slice = (stages + S - 1) / S;
    return (int)((stages + per_slice - 1) / per_slice);
}

// 8 nibbles (one code word: 8 consecutive k) -> their int8 image entries in k order, for a book of at most 16 values whose
// image is the 16 bytes T[0] .. T[3]
__device__ __forceinline__ void i8_decode_word(uint32_t w, const uint32_t (&T)[4], uint32_t &o0, uint32_t &o1)
{
    const uint32_t e7 = w & 0x07070707u, o7 = (w >> 4) & 0x07070707u;                    // elements 0, 2, 4, 6 / 1, 3, 5, 7
    const uint32_t se = ((w >> 1) & 0x04040404u) | 0x03020100u;                          // byte i: i + 4 (bit 3 of the nibble)
    const uint32_t so = ((w >> 5) & 0x04040404u) | 0x03020100u;
    const uint32_t ev = __builtin_amdgcn_perm(__builtin_amdgcn_perm(T[3], T[2], e7), __builtin_amdgcn_perm(T[1], T[0], e7), se);
    const uint32_t od = __builtin_amdgcn_perm(__builtin_amdgcn_perm(T[3], T[2], o7), __builtin_amdgcn_perm(T[1], T[0], o7), so);
    o0 = __builtin_amdgcn_perm(od, ev, 0x05010400u);
    o1 = __builtin_amdgcn_perm(od, ev, 0x07030602u);
}

// the int8 pair of code byte b under the decoder's pair rule (dec_pair): identifier 15 in one nibble -- that element is the
// victim (0), its partner an outlier; g: the image, zero beyond m
__device__ __forceinline__ uint16_t i8_pair_entry(uint32_t b, const uint8_t *g, uint32_t n_normal)
{
    const uint32_t c0 = b & 15u, c1 = b >> 4;
    const uint32_t v0 = (c0 == 15u) ? 0u : g[(c1 == 15u) ? n_normal + c0 : c0];
    const uint32_t v1 = (c1 == 15u) ? 0u : g[(c0 == 15u) ? n_normal + c1 : c1];
    return (uint16_t)(v0 | (v1 << 8));
}

// The constants of a (WAVES, MT) tile that the kernels and their A sides share
template <int WAVES, int MT>
struct I8Tile {
    static constexpr int WR = 16 * MT;                 // rows of xq per wavefront
    static constexpr int BM = WR * WAVES, NTH = 64 * WAVES;
    static constexpr int PIECES = kGemmBK / 16;        // 16-byte pieces of a row of xq per stage
    static constexpr int XL = BM * PIECES / NTH;       // pieces of xq a thread stages per stage
    static constexpr int RSTEP = NTH / PIECES;         // rows between a thread's pieces
};

// The A side of k_linear_i8 itself: xq is a row-major [M, K] matrix, read by i8_tile's own load_x.  Any other A side is a
// type with load(xq, xn), called once per stage in order, which fills the thread's XL pieces of that stage (antq_k_conv_i8.h).
struct I8Matrix { static constexpr bool kFill = false; };

// One tile of S = A . V^T and its epilogue, as the header states it: everything of k_linear_i8 but where a piece of the A
// operand comes from: a row-major matrix xq [M, K] (XS = I8Matrix), or whatever xs.load(xq, xn) gathers for the next stage
// (antq_k_conv_i8.h: im2col).  y is [M, N] row-major.
template <typename T, bool OVP, int WAVES, int MT, typename XS>
__device__ __forceinline__ ANTQ_I8_KERNEL void
i8_tile(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
        uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha_w, int per_row, int I_w, const int8_t *__restrict__ image_w, uint32_t m, int n_normal,
        const float *__restrict__ alpha_x, int I_x, XS &xs)
{
    using TL = I8Tile<WAVES, MT>;
    constexpr int NT = kGemmBN / 16;                   // a wavefront's tiles of 16 output rows
    constexpr int WR = TL::WR, BM = TL::BM, NTH = TL::NTH, PIECES = TL::PIECES, XL = TL::XL, RSTEP = TL::RSTEP;
    constexpr int CL = 256 / NTH;                      // pieces of codes a thread decodes per stage
    constexpr uint32_t BSLOTS = 2u * NT * 64u;         // 16-byte slots of one B image
    static_assert((WAVES == 2 || WAVES == 4) && (MT == 2 || MT == 4) && PIECES == 8 && XL == 2 * MT && kGemmBK == 64 * 2 && NT == 4,
                  "the maps below");
    struct Lds {
        u32x4_t xs[BM * PIECES];                       // the staged xq: piece p of row r at [8 r + (p ^ (r & 7))]
        u32x4_t b[2][BSLOTS];                          // the B images: fragment (j, nt), lane (col, kg) at [((4 j + nt) 4 + kg) 16 + (col ^ (4 j + (kg & 2)))]
        uint16_t pair[256];                            // (pair rule) the int8 pair of a code byte
        __attribute__((aligned(16))) uint8_t g[32];    // the image, zero beyond m (dec4_book's padding)
    };
    __shared__ Lds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t n0 = blockIdx.x * (uint32_t)kGemmBN, m0 = blockIdx.y * (uint32_t)BM;
    const uint32_t nstages = (K + (uint32_t)kGemmBK - 1u) / (uint32_t)kGemmBK;
    const bool active = m0 + (uint32_t)WR * wave < M;  // (wave-uniform) this wavefront has rows of xq
    const size_t row_bytes = (size_t)(K >> 1);

    // this thread's pieces of xq: piece tid & 7 of rows (tid >> 3) + RSTEP i
    const uint32_t xp = tid & 7u, xr0 = tid >> 3;
    u32x4_t xn[XL];
    auto load_x = [&](uint32_t c) __attribute__((always_inline)) {
        if constexpr (std::is_same<XS, I8Matrix>::value) {
            const uint32_t k0 = c * (uint32_t)kGemmBK + 16u * xp;
            const bool kok = k0 < K;
            const size_t koff = (size_t)min(k0, K - 16u);
#pragma unroll
            for (int i = 0; i < XL; i++) {
                const uint32_t r = m0 + xr0 + (uint32_t)(RSTEP * i);
                u32x4_t v = *(const ANTQ_GLOBAL u32x4_t *)(reinterpret_cast<const char *>(xq) + (size_t)min(r, M - 1u) * K + koff);
                if (!(kok && r < M)) v = u32x4_t{0u, 0u, 0u, 0u};
                xn[i] = v;
            }
        } else xs.load(xq, xn);
    };
    auto write_x = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t r = xr0 + (uint32_t)(RSTEP * i);
            lds.xs[r * PIECES + (xp ^ (r & 7u))] = xn[i];
        }
    };
    // the pieces of codes of stage c: one with n >= N or k >= K loads nothing
    auto load_codes = [&](uint32_t c, u32x4_t (&w)[CL]) __attribute__((always_inline)) {
#pragma unroll
        for (int l = 0; l < CL; l++) {
            const uint32_t q = tid + (uint32_t)(NTH * l), n = n0 + (q >> 2), k0 = c * (uint32_t)kGemmBK + 32u * (q & 3u);
            w[l] = u32x4_t{0u, 0u, 0u, 0u};
            if (n < N && k0 < K)
                w[l] = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(reinterpret_cast<const char *>(codes) + (size_t)n * row_bytes + (k0 >> 1)));
        }
    };

    // __syncthreads(), spelled out: a function without this kernel's target attribute is not inlined into it
    auto sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };

    u32x4_t cw[CL], cwn[CL];
    load_x(0u);                                        // in flight while the tables are built
    load_codes(0u, cw);
    load_codes(1u, cwn);
    if (tid < 32u) lds.g[tid] = tid < m ? (uint8_t)image_w[tid] : (uint8_t)0;
    sync();
    uint32_t img[4] = {0u, 0u, 0u, 0u};
    if constexpr (OVP) {
        for (uint32_t b = tid; b < 256u; b += (uint32_t)NTH) lds.pair[b] = i8_pair_entry(b, lds.g, (uint32_t)n_normal);
        sync();
    } else {
        const u32x4_t t = *reinterpret_cast<const u32x4_t *>(lds.g);
        img[0] = t.x; img[1] = t.y; img[2] = t.z; img[3] = t.w;
    }

    // piece l of this thread, stage c: 32 nibbles -> two operands of 16 int8, into B image c & 1
    auto decode_write = [&](uint32_t c, int l) __attribute__((always_inline)) {
        const uint32_t q = tid + (uint32_t)(NTH * l), n = q >> 2, qk = q & 3u;
        const uint32_t wd[4] = {cw[l].x, cw[l].y, cw[l].z, cw[l].w};
        uint32_t o[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if constexpr (OVP) {
                o[2 * i] = (uint32_t)lds.pair[wd[i] & 0xffu] | ((uint32_t)lds.pair[(wd[i] >> 8) & 0xffu] << 16);
                o[2 * i + 1] = (uint32_t)lds.pair[(wd[i] >> 16) & 0xffu] | ((uint32_t)lds.pair[wd[i] >> 24] << 16);
            } else i8_decode_word(wd[i], img, o[2 * i], o[2 * i + 1]);
        }
        // (a piece that loaded nothing holds code 0 everywhere, whose entry need not be 0)
        const bool ok = n0 + n < N && c * (uint32_t)kGemmBK + 32u * qk < K;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            u32x4_t v = u32x4_t{o[4 * h], o[4 * h + 1], o[4 * h + 2], o[4 * h + 3]};
            if (!ok) v = u32x4_t{0u, 0u, 0u, 0u};
            const uint32_t j = qk >> 1, g = 2u * (qk & 1u) + (uint32_t)h;
            lds.b[c & 1u][((4u * j + (n >> 4)) * 4u + g) * 16u + ((n & 15u) ^ (4u * j + (g & 2u)))] = v;
        }
    };

    i32x4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = i32x4_t{0, 0, 0, 0};

    // MFMA step j of stage c: k = 128 c + 64 j + 16 kg .. + 15
    auto mfma_step = [&](uint32_t c, int j) __attribute__((always_inline)) {
        i32x4_t b[NT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
            b[nt] = __builtin_bit_cast(i32x4_t, lds.b[c & 1u][((4u * j + nt) * 4u + kg) * 16u + (col ^ (4u * j + (kg & 2u)))]);
        const uint32_t p = 4u * j + kg;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const i32x4_t a = __builtin_bit_cast(i32x4_t, lds.xs[((uint32_t)WR * wave + 16u * mt + col) * PIECES + (p ^ (col & 7u))]);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[nt], acc[mt][nt], 0, 0, 0);
        }
    };

    // stage 0: decoded and staged before the loop
#pragma unroll
    for (int l = 0; l < CL; l++) decode_write(0u, l);
    write_x();

    for (uint32_t c = 0; c < nstages; c++) {
        sync();                               // xq image and B image of stage c written
        const bool more = c + 1u < nstages;
#pragma unroll
        for (int l = 0; l < CL; l++) cw[l] = cwn[l];
        if (more) {
            load_x(c + 1u);
            load_codes(c + 2u, cwn);
            // the decode of stage c + 1 beside the MFMAs of stage c
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (j < CL) decode_write(c + 1u, j);
                if (active) mfma_step(c, j);
            }
        } else if (active) {
#pragma unroll
            for (int j = 0; j < 2; j++) mfma_step(c, j);
        }
        if (!more) break;
        sync();                               // the xq image free again
        write_x();
    }

    // C / D map: column (n) = lane & 15, row (m) = 4 (lane >> 4) + reg
    if (!active) return;
    const float u_x = ld_global(alpha_x) / (float)I_x;
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const uint32_t n = n0 + 16u * nt + col;
        if (n >= N) continue;
        const float u_w = ld_global(alpha_w + (per_row ? n : 0u)) / (float)I_w;
        const float bv = bias ? IO<T>::load1(bias, n) : 0.0f;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + (uint32_t)WR * wave + 16u * mt + 4u * kg + r;
                if (mrow < M) {
                    float v = (float)acc[mt][nt][r];
                    v = v * u_x;
                    v = v * u_w;
                    if (bias) v = v + bv;
                    IO<T>::store1(y, (size_t)mrow * N + n, v);
                }
            }
    }
}

template <typename T, bool OVP, int WAVES, int MT>
__global__ void __launch_bounds__(64 * WAVES) ANTQ_I8_KERNEL
k_linear_i8(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
            uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha_w, int per_row, int I_w,
            const int8_t *__restrict__ image_w, uint32_t m, int n_normal, const float *__restrict__ alpha_x, int I_x)
{
    I8Matrix xs;
    i8_tile<T, OVP, WAVES, MT>(codes, xq, bias, y, M, N, K, alpha_w, per_row, I_w, image_w, m, n_normal, alpha_x, I_x, xs);
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR_I8_H
