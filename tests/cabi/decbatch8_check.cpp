// The byte-code decoder's pure-host blob builder (ant_quantization_amd/csrc/antq_decbatch8.h) on its own: no HIP, no
// library, no Python.  Meant to be compiled with -fsanitize=address,undefined (tests/test_byte_codes_host.py does) and fed
// the refusals and the edge jobs: every blob is built into a heap buffer of EXACTLY the size the capacity call named, so a
// write one byte past it is an error report, not a silent pass.  Exit code 0 and a last line "ok": every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ant_quantization_amd/csrc/antq_decbatch8.h"

using namespace antq;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static const uintptr_t FAKE = 0x7f0000000000ull;      // the builder only looks at addresses: nothing is dereferenced

static antq_decode_job job(size_t rows, size_t row_len, int per_row = 1, int m = 256, int n_normal = 0, uintptr_t codes = FAKE,
                           uintptr_t out = FAKE + (1u << 20))
{
    antq_decode_job J;
    memset(&J, 0, sizeof(J));
    J.codes_dev = reinterpret_cast<const uint8_t *>(codes);
    J.out_dev = reinterpret_cast<void *>(out);
    J.alpha_dev = reinterpret_cast<const float *>(FAKE + (2u << 20));
    J.grid_dev = reinterpret_cast<const float *>(FAKE + (3u << 20));
    J.rows = rows; J.row_len = row_len; J.alpha_per_row = per_row; J.gmax = 10.0f; J.m = m; J.n_normal = n_normal;
    return J;
}

// build into an exact-size heap buffer; returns the builder's answer, the blob in `blob`
static int build(const std::vector<antq_decode_job> &jobs, int dtype, unsigned flags, std::vector<uint8_t> *blob = nullptr, long shrink = 0)
{
    const size_t cap = dec8_batch_capacity(jobs.data(), (int)jobs.size(), dtype);
    const size_t have = cap > (size_t)shrink ? cap - (size_t)shrink : 0;
    uint8_t *buf = static_cast<uint8_t *>(malloc(have ? have : 1));
    const int n = dec8_batch_build(jobs.data(), (int)jobs.size(), dtype, flags, buf, have);
    if (n > 0 && blob) blob->assign(buf, buf + n);
    free(buf);
    return n;
}

static DecDesc desc_of(const std::vector<uint8_t> &blob, int i)
{
    DecDesc D;
    memcpy(&D, blob.data() + sizeof(DecHeader) + sizeof(DecDesc) * (size_t)i, sizeof(D));
    return D;
}

int main()
{
    // refusals, each with its code
    CHECK(build({job(4, 64)}, ANTQ_BF16, 0) > 0);
    CHECK(build({job(4, 64), job(4, 6)}, ANTQ_BF16, 0) == ANTQ_ERR_UNSUPPORTED);            // row_len % 4 != 0
    CHECK(build({job(4, 147)}, ANTQ_F32, 0) == ANTQ_ERR_UNSUPPORTED);
    CHECK(build({job(4, 64, 1, 257)}, ANTQ_BF16, 0) == ANTQ_ERR_UNSUPPORTED);               // 257 plain values
    CHECK(build({job(4, 64, 1, 510, 255)}, ANTQ_BF16, ANTQ_FLAG_OVP) > 0);                  // 255 + 255
    CHECK(build({job(4, 64, 1, 509, 255)}, ANTQ_BF16, ANTQ_FLAG_OVP) > 0);                  // OliVe int-8
    CHECK(build({job(4, 64, 1, 511, 256)}, ANTQ_BF16, ANTQ_FLAG_OVP) == ANTQ_ERR_UNSUPPORTED);
    CHECK(build({job(4, 64, 1, 511, 255)}, ANTQ_BF16, ANTQ_FLAG_OVP) == ANTQ_ERR_UNSUPPORTED);   // 256 outliers
    CHECK(build({job(4, 64, 1, 20, 0)}, ANTQ_BF16, ANTQ_FLAG_OVP) == ANTQ_ERR_UNSUPPORTED);
    CHECK(build({job(4, 64, 1, 20, 21)}, ANTQ_BF16, ANTQ_FLAG_OVP) == ANTQ_ERR_UNSUPPORTED);
    CHECK(build({job(4, 64, 1, 255, 255)}, ANTQ_BF16, ANTQ_FLAG_OVP) > 0);                  // no outliers at all
    CHECK(build({job(4, 64, 1, 0)}, ANTQ_BF16, 0) == ANTQ_ERR_ARG);
    CHECK(build({job(0, 64)}, ANTQ_BF16, 0) == ANTQ_ERR_ARG);                               // empty
    CHECK(build({job(4, 0)}, ANTQ_BF16, 0) == ANTQ_ERR_ARG);
    CHECK(build({job(4, 64, 1, 256, 0, 0)}, ANTQ_BF16, 0) == ANTQ_ERR_ARG);                 // null codes
    CHECK(build({job(4, 64, 1, 256, 0, FAKE, 0)}, ANTQ_BF16, 0) == ANTQ_ERR_ARG);           // null out
    {
        antq_decode_job J = job(4, 64);
        J.alpha_dev = nullptr;
        CHECK(build({J}, ANTQ_BF16, 0) == ANTQ_ERR_ARG);
        J = job(4, 64);
        J.grid_dev = nullptr;
        CHECK(build({J}, ANTQ_BF16, 0) == ANTQ_ERR_ARG);
    }
    CHECK(build({job(4, 64, 1, 256, 0, FAKE, FAKE + (1u << 20) + 1)}, ANTQ_BF16, 0) == ANTQ_ERR_ALIGN);
    CHECK(build({job(4, 64, 1, 256, 0, FAKE, FAKE + (1u << 20) + 2)}, ANTQ_F32, 0) == ANTQ_ERR_ALIGN);
    CHECK(build({job(4, 64, 1, 256, 0, FAKE, FAKE + (1u << 20) + 2)}, ANTQ_BF16, 0) > 0);
    CHECK(build({job(4, 64)}, ANTQ_BF16, 2) == ANTQ_ERR_ARG);                               // a flag other than the pair rule
    CHECK(build({job(4, 64)}, ANTQ_BF16, ANTQ_FLAG_OVP | 4u) == ANTQ_ERR_ARG);
    CHECK(build({job(4, 64)}, ANTQ_F64, 0) == ANTQ_ERR_UNSUPPORTED);
    CHECK(build({job(4, 64)}, 9, 0) == ANTQ_ERR_UNSUPPORTED);
    CHECK(build({job(4, 64)}, ANTQ_BF16, 0, nullptr, 1) == ANTQ_ERR_PLAN);                  // one byte short
    CHECK(build({job(4, 64), job(700, 4100)}, ANTQ_F32, 0, nullptr, 4) == ANTQ_ERR_PLAN);
    CHECK(dec8_batch_capacity(nullptr, 1, ANTQ_BF16) == 0);
    CHECK(dec8_batch_capacity(std::vector<antq_decode_job>{job(4, 64)}.data(), 0, ANTQ_BF16) == 0);
    {
        uint8_t b[64];
        antq_decode_job J = job(4, 64);
        CHECK(dec8_batch_build(nullptr, 1, ANTQ_BF16, 0, b, sizeof(b)) == ANTQ_ERR_ARG);
        CHECK(dec8_batch_build(&J, 1, ANTQ_BF16, 0, nullptr, 4096) == ANTQ_ERR_ARG);
        CHECK(dec8_batch_build(&J, 0, ANTQ_BF16, 0, b, sizeof(b)) == ANTQ_ERR_ARG);
        CHECK(dec8_batch_build(&J, 65536, ANTQ_BF16, 0, b, sizeof(b)) == ANTQ_ERR_ARG);
    }

    // task counts at every edge, the kinds, the map; every dtype
    for (int dtype : {ANTQ_F32, ANTQ_BF16, ANTQ_F16}) {
        const size_t epl = dtype == ANTQ_F32 ? 4 : 8;
        std::vector<size_t> lens = {4, 8, 12, 20, 252, 256, 260, 1024, 4100};
        for (size_t v : {127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513}) lens.push_back(v * epl);
        for (size_t rows : {1, 3, 257}) {
            std::vector<antq_decode_job> jobs;
            for (size_t rl : lens) {
                jobs.push_back(job(rows, rl, 1));
                jobs.push_back(job(rows, rl, 0));
                jobs.push_back(job(rows, rl, 1, 256, 0, FAKE + 1 + rl % 3));                  // codes off a word
                jobs.push_back(job(rows, rl, 1, 256, 0, FAKE, FAKE + (1u << 20) + epl));       // out off a 16-byte vector
            }
            // flat element counts around the tasks of the two per-lane kinds (256 vectors / 256 quads)
            for (size_t units : {255, 256, 257, 511, 512, 513}) {
                jobs.push_back(job(units, epl, 1));
                jobs.push_back(job(units, 4, 1, 256, 0, FAKE + 2));
            }
            std::vector<uint8_t> blob;
            const int n = build(jobs, dtype, 0, &blob);
            CHECK(n > 0);
            if (n <= 0) continue;
            DecHeader h;
            memcpy(&h, blob.data(), sizeof(h));
            CHECK(h.magic == kDec8Magic && h.n == jobs.size() && (int)h.bytes == n && h.dtype == (uint32_t)dtype);
            uint32_t first = 0;
            for (size_t i = 0; i < jobs.size(); i++) {
                const antq_decode_job &J = jobs[i];
                const DecDesc D = desc_of(blob, (int)i);
                const size_t n_el = J.rows * J.row_len;
                const size_t rl = J.alpha_per_row ? J.row_len : n_el, rws = J.alpha_per_row ? J.rows : 1;
                const bool aligned = reinterpret_cast<uintptr_t>(J.codes_dev) % 4 == 0 && reinterpret_cast<uintptr_t>(J.out_dev) % 16 == 0 && rl % epl == 0;
                size_t want;
                if (!aligned) {
                    CHECK(D.kind == kDec8Quad && D.n_units == n_el / 4 && D.vpr == rl / 4);
                    want = (n_el / 4 + 255) / 256;
                } else if (rl / epl >= 128) {
                    CHECK(D.kind == kDec8Row && D.u >= 2 && D.u <= 4 && D.vpr == rl / epl);
                    CHECK(D.tpr == (rl / epl + 64 * D.u - 1) / (64 * D.u));
                    want = rws * D.tpr;
                } else {
                    CHECK(D.kind == kDec8Lane && D.n_units == n_el / epl && D.vpr == rl / epl);
                    want = (n_el / epl + 255) / 256;
                }
                CHECK(D.total_tasks == want && D.first_block == first && D.m == 256 && D.n_normal == 0);
                for (uint32_t b = 0; b < (D.total_tasks + 3) / 4; b++) {
                    uint32_t j;
                    memcpy(&j, blob.data() + h.map_offset + 4 * (size_t)(first + b), 4);
                    CHECK(j == i);
                }
                first += (D.total_tasks + 3) / 4;
            }
            CHECK(first == h.total_blocks && h.map_offset + 4 * (size_t)first == (size_t)n);
        }
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
