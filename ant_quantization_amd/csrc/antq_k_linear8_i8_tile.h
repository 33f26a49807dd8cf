// antq_k_linear8_i8_tile.h -- NOT a header of its own: the body of the tiled byte-code kernels, included INSIDE k_linear8_i8
// (antq_k_linear8_i8.h) and k_conv2d8_i8 (antq_k_conv8_i8.h), which differ in the A side alone.  Textual, not a function: moved
// into an inlined function the same statements compile to other control flow, and k_linear8_i8 has to keep its instructions.
// The including kernel provides T, TABLE, WAVES, MT, the type XS and the object xs (I8Matrix: xq is a row-major [M, K] matrix; else
// xs.load(xq, xn) gathers the next stage's pieces, asked in order from stage 0), the kernel arguments of k_linear8_i8 under
// their names, and wsum: with XS::kFill and wsum not null the integer 128 wsum[n] is added to every sum of column n in the
// epilogue (the offset form of antq_conv2d8_i8); without kFill there is no such code.
    constexpr int NT = kGemmBN / 16;                   // a wavefront's tiles of 16 output rows
    constexpr int WR = 16 * MT;                        // rows of xq per wavefront
    constexpr int BM = WR * WAVES, NTH = 64 * WAVES;
    constexpr int PIECES = kGemmBK / 16;               // 16-byte pieces of a row (of xq, of codes) per stage
    constexpr int XL = BM * PIECES / NTH;              // pieces of xq a thread stages per stage
    constexpr int RSTEP = NTH / PIECES;                // rows between a thread's pieces
    constexpr int CL = kGemmBN * PIECES / NTH;         // pieces of codes a thread forwards per stage
    constexpr uint32_t BSLOTS = 2u * NT * 64u;         // 16-byte slots of one B image
    static_assert((WAVES == 2 || WAVES == 4) && (MT == 2 || MT == 4) && PIECES == 8 && XL == 2 * MT && kGemmBK == 64 * 2 && NT == 4 &&
                  CL % 2 == 0, "the maps below");
    struct Lds {
        u32x4_t xs[BM * PIECES];                       // the staged xq: piece p of row r at [8 r + (p ^ (r & 7))]
        u32x4_t b[2][BSLOTS];                          // the B images: fragment (j, nt), lane (col, kg) at [((4 j + nt) 4 + kg) 16 + (col ^ (4 j + kg) ^ 8 (col & 1))]
        __attribute__((aligned(16))) uint8_t tab[256]; // (TABLE) the int8 of a code byte, zero beyond m
    };
    __shared__ Lds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t n0 = blockIdx.x * (uint32_t)kGemmBN, m0 = blockIdx.y * (uint32_t)BM;
    const uint32_t nstages = (K + (uint32_t)kGemmBK - 1u) / (uint32_t)kGemmBK;
    const bool active = m0 + (uint32_t)WR * wave < M;  // (wave-uniform) this wavefront has rows of xq

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
        } else xs.load(xq, xn);                        // (the stages 0, 1, ... in order)
    };
    auto write_x = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t r = xr0 + (uint32_t)(RSTEP * i);
            lds.xs[r * PIECES + (xp ^ (r & 7u))] = xn[i];
        }
    };
    // this thread's pieces of codes: piece cp = tid & 7 of the tile's rows (tid >> 3) + RSTEP l (q = tid + NTH l).  Loaded
    // from a clamped address whatever n and k; piece_ok says whether it counts.
    const uint32_t cp = tid & 7u, cr0 = tid >> 3;
    auto piece_ok = [&](uint32_t c, int l) __attribute__((always_inline)) {
        return n0 + cr0 + (uint32_t)(RSTEP * l) < N && c * (uint32_t)kGemmBK + 16u * cp < K;
    };
    auto load_codes = [&](uint32_t c, u32x4_t (&w)[CL]) __attribute__((always_inline)) {
        const size_t koff = (size_t)min(c * (uint32_t)kGemmBK + 16u * cp, K - 16u);
#pragma unroll
        for (int l = 0; l < CL; l++) {
            const uint32_t n = min(n0 + cr0 + (uint32_t)(RSTEP * l), N - 1u);
            w[l] = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(reinterpret_cast<const char *>(codes) + (size_t)n * K + koff));
        }
    };

    // __syncthreads(), spelled out: a function without this kernel's target attribute is not inlined into it
    auto sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };

    u32x4_t cw[CL], cwn[CL];
    load_x(0u);                                        // in flight while the table is built
    load_codes(0u, cw);
    load_codes(1u, cwn);
    if constexpr (TABLE) {
        for (uint32_t b = tid; b < 256u; b += (uint32_t)NTH) lds.tab[b] = b < m ? (uint8_t)image_w[b] : (uint8_t)0;
        sync();
    }

    // piece l of this thread, stage c: its 16 codes -> one operand of 16 int8, into B image c & 1
    auto decode_write = [&](uint32_t c, int l) __attribute__((always_inline)) {
        const uint32_t n = cr0 + (uint32_t)(RSTEP * l), ncol = n & 15u;
        u32x4_t v = i8b_operand<TABLE>(cw[l], lds.tab);
        // (a piece that does not count: exact zeros, not the entry of whatever code was loaded)
        if (!piece_ok(c, l)) v = u32x4_t{0u, 0u, 0u, 0u};
        const uint32_t j = cp >> 2, g = cp & 3u;
        lds.b[c & 1u][((4u * j + (n >> 4)) * 4u + g) * 16u + (ncol ^ cp ^ (8u * (ncol & 1u)))] = v;
    };

    i32x4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = i32x4_t{0, 0, 0, 0};

    // MFMA step j of stage c: k = 128 c + 64 j + 16 kg .. + 15
    auto mfma_step = [&](uint32_t c, int j) __attribute__((always_inline)) {
        i32x4_t b[NT];
        const uint32_t p = 4u * j + kg;
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
            b[nt] = __builtin_bit_cast(i32x4_t, lds.b[c & 1u][((4u * j + nt) * 4u + kg) * 16u + (col ^ p ^ (8u * (col & 1u)))]);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const i32x4_t a = __builtin_bit_cast(i32x4_t, lds.xs[((uint32_t)WR * wave + 16u * mt + col) * PIECES + (p ^ (col & 7u))]);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[nt], acc[mt][nt], 0, 0, 0);
        }
    };

    // stage 0: written and staged before the loop
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
            // the B image of stage c + 1 beside the MFMAs of stage c
#pragma unroll
            for (int j = 0; j < 2; j++) {
#pragma unroll
                for (int l = j * (CL / 2); l < (j + 1) * (CL / 2); l++) decode_write(c + 1u, l);
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
        int corr = 0;                         // (the offset form) 128 wsum[n]: an integer add in the epilogue, no register in the loop
        if constexpr (XS::kFill) corr = wsum ? wsum[n] * 128 : 0;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + (uint32_t)WR * wave + 16u * mt + 4u * kg + r;
                if (mrow < M) i8_sk_store<T>(y, (size_t)mrow * N + n, acc[mt][nt][r] + corr, u_x, u_w, bias != nullptr, bv);
            }
    }
