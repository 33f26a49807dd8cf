// antq_k_quant_nhwc.h -- transposing quantiser (antq_quant_i8_nhwc): a contiguous NCHW activation [B, C, P = H W] to the int8
// image of its codes in NHWC order [B, P, C], what antq_conv2d4_i8 reads, in one pass -- 4 + 1 bytes per fp32 element where
// contiguous(channels_last) + antq_quant_i8 move 4 + 4 + 4 + 1.
// Part of libantq's single device translation unit (antq_kernels.hip includes it); gfx950 only.
//
// The decisions are antq_quant_i8's, element for element: encode_unit_a (plans with adom) or quant_vec + k_encode's code
// mapping, both with their literal paths, and the CodeI8 store trait (512-byte image table, stage / map) without the pair
// rule.  With one scale and no pair rule a byte depends on its element alone, so which 8 elements share a unit cannot
// change a bit: here a unit is 8 positions of ONE channel, which is what the reads want.
//
//   tile       64 channels x 128 positions of one image; 256 threads, thread (cg = tid / 16, pg = tid % 16) owns channels
//              4 cg .. 4 cg + 3 and eight positions: slot j of position group pg is position
//                  pos(pg, j) = (j / EPL) * 16 EPL + pg * EPL + j % EPL          (EPL = 4 fp32, 8 bf16 / f16)
//              -- fp32: two quads 64 positions apart, 16-bit: one octet -- so that the 16 lanes of a channel read one
//              contiguous 256-byte run per load instruction.  128 positions in every dtype: 4 channels x 8 positions is the
//              unit the register transpose needs, and 8 (fp32) / 4 (16-bit) 16-byte loads per thread are in flight before
//              the first use.  Workgroups are persistent (the plan's table and the image table are staged once) and walk
//              the tiles position tile fastest, then channel slab, then image.
//   reads      VEC: 16-byte nontemporal loads along P; holds when x is 16-byte aligned and P * sizeof(T) % 16 == 0 (every
//              channel row then starts aligned and a vector is wholly inside or outside P).  Else element loads with the
//              same ownership.  The launcher picks; masked lanes load nothing and encode zeros that are never stored.
//   transpose  the 4 x 8 finished bytes of a thread, one word of 4 positions per channel and half, become 8 words of 4
//              channels each through v_perm_b32 (8 per 4 x 4 block), and go to the int8 LDS tile as ds_write_b32.
//   LDS tile   128 rows of 64 bytes, no padding; slot (pg, j) lives in row j * 16 + (pg ^ (j & 3)), and 16-byte piece k of a
//              row (channels 16 k .. 16 k + 15) at piece k ^ (pg >> 2).  Bank of a word = 16 (row % 4) + 4 piece + word:
//              a write instruction (j fixed; pg = 0 .. 15, 4 consecutive words of one piece w) hits 16 ((pg ^ j) & 3) +
//              4 (w ^ (pg >> 2)) + word -- 64 different banks; a read instruction (16 consecutive positions, all 4 pieces)
//              reads 16 whole rows, 4 of every row phase -- 4 words per bank, the minimum of 1 KiB over 64 banks.
//              Two tiles alternate, so ONE barrier per tile orders everything: a thread that writes buffer t & 1 for tile
//              t + 2 has passed the barrier of tile t + 1, which every thread reaches only after its reads of tile t.
//   writes     lane (tid / 4 + 64 s, tid % 4), s = 0, 1: one ds_read_b128 and one 16-byte nontemporal store to
//              q + (b P + p) C + c0 + 16 k; a wavefront's store covers 16 positions x 64 bytes, one 1 KiB run when C = 64.
#ifndef ANTQ_K_QUANT_NHWC_H
#define ANTQ_K_QUANT_NHWC_H

#include "antq_k_codec8.h"

namespace antq {

constexpr int kNhwcCh = 64;                            // channels of a tile
constexpr int kNhwcPos = 128;                          // positions of a tile

// the four words {a, b, c, d} (byte i of each: position i of one channel) -> o[i] = bytes a_i b_i c_i d_i (4 channels of position i)
__device__ __forceinline__ void nhwc_transpose4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t *o)
{
    const uint32_t ab01 = __builtin_amdgcn_perm(b, a, 0x05010400u), ab23 = __builtin_amdgcn_perm(b, a, 0x07030602u);
    const uint32_t cd01 = __builtin_amdgcn_perm(d, c, 0x05010400u), cd23 = __builtin_amdgcn_perm(d, c, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(cd01, ab01, 0x05040100u);
    o[1] = __builtin_amdgcn_perm(cd01, ab01, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(cd23, ab23, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(cd23, ab23, 0x07060302u);
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
k_quant_i8_nhwc(const void *__restrict__ x, int8_t *__restrict__ q, uint32_t C, uint32_t P, uint32_t npt, uint32_t nct, uint32_t n_tiles,
                const float *__restrict__ alpha, float gmax, int zero_code, PlanArgs pa, const uint4 *__restrict__ plan_tab,
                QuantI8Arg img)
{
    constexpr int EPL = IO<T>::EPL;
    constexpr int NV = 8 / EPL;                        // 16-byte vectors per channel and thread
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    __shared__ __attribute__((aligned(16))) uint4 tile[2][kNhwcPos * kNhwcCh / 16];
    uint4 tab0 = make_uint4(0, 0, 0, 0);
    if (pa.adom) tab0 = atab_prefetch<true>(pa, plan_tab);
    else if (threadIdx.x < pa.tab_units) tab0 = plan_tab[threadIdx.x];
    PlanLds L;
    ATab A;
    if (pa.adom) {
        A = stage_atab<true>(pa, plan_tab, smem, tab0);
        __syncthreads();
        atab_to_codes<false, 255u>(pa, smem, A, 0);
    } else L = stage_plan(pa, plan_tab, smem, tab0);
    CodeI8::stage<false>(img, 0);
    __syncthreads();
    const float a0 = alpha[0];
    const double inv_gmax = 1.0 / (double)gmax;
    const ScaleA sa = make_scale_a(a0, gmax, inv_gmax);
    const Scale sc = make_scale(a0, gmax);
    const uint32_t pg = threadIdx.x & 15u, cg = threadIdx.x >> 4;
    // this thread's word of slot j: row j * 16 + (pg ^ (j & 3)), piece (cg >> 2) ^ (pg >> 2), word cg & 3
    const uint32_t wcol = ((((cg >> 2) ^ (pg >> 2)) << 2) | (cg & 3u));
    uint32_t buf = 0;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x, buf ^= 1u) {
        const uint32_t pt = t % npt, r = t / npt, ct = r % nct, b = r / nct;
        const uint32_t p0 = pt * kNhwcPos, c0 = ct * kNhwcCh;
        float xf[4][8];
        if constexpr (VEC) {
            uint4 v[4][NV];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t c = c0 + 4u * cg + k;
#pragma unroll
                for (int h = 0; h < NV; h++) {
                    const uint32_t p = p0 + h * 16 * EPL + pg * EPL;
                    v[k][h] = make_uint4(0, 0, 0, 0);
                    if (c < C && p < P)                // (P % EPL == 0: the vector is wholly inside)
                        v[k][h] = ld_stream(reinterpret_cast<const uint4 *>(static_cast<const char *>(x) +
                                                                            (((size_t)b * C + c) * P + p) * IO<T>::ESIZE));
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if constexpr (NV == 1) IO<T>::unpack(v[k][0], xf[k]);
                else {
                    float lo[4], hi[4];
                    IO<T>::unpack(v[k][0], lo);
                    IO<T>::unpack(v[k][1], hi);
#pragma unroll
                    for (int e = 0; e < 4; e++) { xf[k][e] = lo[e]; xf[k][4 + e] = hi[e]; }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t c = c0 + 4u * cg + k;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const uint32_t p = p0 + (j / EPL) * 16 * EPL + pg * EPL + j % EPL;
                    xf[k][j] = (c < C && p < P) ? IO<T>::load1(x, ((size_t)b * C + c) * P + p) : 0.0f;
                }
            }
        }
        uint32_t w[4][2];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (pa.adom) encode_unit_a<CodeI8, false, 8>(pa, A.tab, A.grid, sa, xf[k], 0, zero_code, w[k]);
            else {
                float of[8];
                int jx[8];
                quant_vec<8, false, true>(pa, L, sc, xf[k], of, jx);
                uint32_t cc[8];
#pragma unroll
                for (int e = 0; e < 8; e++) cc[e] = jx[e] == ANTQ_IDX_NONE ? (uint32_t)zero_code : (uint32_t)jx[e];
                CodeI8::pack<false>(cc, w[k]);
            }
        }
        uint32_t o[8];
        nhwc_transpose4(w[0][0], w[1][0], w[2][0], w[3][0], o);
        nhwc_transpose4(w[0][1], w[1][1], w[2][1], w[3][1], o + 4);
        uint32_t *tw = reinterpret_cast<uint32_t *>(tile[buf]);
#pragma unroll
        for (int j = 0; j < 8; j++) tw[((uint32_t)j * 16u + (pg ^ (uint32_t)(j & 3))) * (kNhwcCh / 4) + wcol] = o[j];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t pl = s * 64u + (threadIdx.x >> 2), k = threadIdx.x & 3u;
            const uint32_t rpg = (pl % (16 * EPL)) / EPL, rj = (pl / (16 * EPL)) * EPL + pl % EPL;
            const uint4 piece = tile[buf][(rj * 16u + (rpg ^ (rj & 3u))) * 4u + (k ^ (rpg >> 2))];
            const uint32_t p = p0 + pl, c = c0 + 16u * k;
            if (p < P && c < C) st_stream(reinterpret_cast<uint4 *>(q + ((size_t)b * P + p) * C + c), piece);
        }
    }
}

// Sizes checked by the caller: C % 16 == 0, B P C <= ANTQ_QUANT_I8_NHWC_MAX_BYTES, nothing empty.
template <typename T>
static int launch_quant_i8_nhwc(const void *x, int8_t *q, size_t B, size_t C, size_t P, const float *alpha, float gmax, const PlanArgs &pa,
                                const void *plan_host, const void *plan_dev, const int8_t *image, hipStream_t st)
{
    if (!CodeI8::book_ok((int)pa.m, 0, false)) return ANTQ_ERR_UNSUPPORTED;
    const size_t npt = (P + kNhwcPos - 1) / kNhwcPos, nct = (C + kNhwcCh - 1) / kNhwcCh;
    const size_t n_tiles = B * nct * npt;              // <= B P C < 2^31
    const size_t blocks = std::min(n_tiles, (size_t)(g_knob_encwg > 0 ? g_knob_encwg : 2048));
    const bool vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && (P * IO<T>::ESIZE) % 16 == 0;
    const int zero_code = codec_zero_code(plan_host, pa, 0, false);
    const size_t lds = lds_table(pa, true);
    return with_bool(vec, [&](auto v) {
        launch_k(false, k_quant_i8_nhwc<T, decltype(v)::value>, dim3((unsigned)blocks), dim3(256), lds, st, x, q, (uint32_t)C, (uint32_t)P,
                 (uint32_t)npt, (uint32_t)nct, (uint32_t)n_tiles, alpha, gmax, zero_code, pa, plan_tab_ptr(plan_dev),
                 CodeI8::arg(1, image, (int)pa.m));
        return launch_status();
    });
}

}  // namespace antq

#endif  // ANTQ_K_QUANT_NHWC_H
