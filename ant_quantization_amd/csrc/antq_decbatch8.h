// antq_decbatch8.h -- the byte-code decoder's descriptor blob and its pure-host builder (antq_decode8_batch_capacity /
// antq_decode8_batch_build; antq_decode8 builds ONE descriptor with the same rule and passes it by value).  No HIP in this
// file: antq_plan.cpp compiles the builder, the kernels (antq_k_decbatch8.h) read the same structs.
//
// The byte-per-element twin of antq_decbatch.h: the same blob (DecHeader | DecDesc descs[n] | uint32 map[total_blocks], a
// map entry = 4 consecutive one-wavefront tasks of one job), another magic, other task kinds:
//   kDec8Row   rows of >= 128 output vectors (and every per-tensor-scale job that long), codes 4-byte and out 16-byte
//              aligned, the row a whole number of vectors: a task is u x 64 vectors inside ONE row, so one scale -- the
//              wavefront builds a table of 256 finished outputs keyed by the code byte (pair rule: a second one for the
//              outlier list) and every element costs one LDS read
//   kDec8Lane  shorter rows, same alignment: u x 64 vectors of the flat tensor, the scale per lane (a vector never leaves
//              its row), the codebook itself in LDS
//   kDec8Quad  codes not 4-byte or out not 16-byte aligned, or a 16-bit row of 4 mod 8 elements: 64 x 4 quads (4 elements,
//              two pairs: row_len % 4 == 0 keeps a quad inside one row) per task, byte loads and element stores
#ifndef ANTQ_DECBATCH8_H
#define ANTQ_DECBATCH8_H

#include "antq_decbatch.h"

namespace antq {

constexpr uint32_t kDec8Magic = 0x38444E41u;   // "AND8"
constexpr uint32_t kDec8Row = 0, kDec8Lane = 1, kDec8Quad = 2;
constexpr uint32_t kDec8Ident = 255;           // the pair rule's identifier: this element is the victim, its partner an outlier
constexpr uint32_t kDec8QuadU = 4;             // quads per lane and task of the element-granular kind
constexpr uint32_t kDec8LaneU = 4;             // vectors per lane and task of the short-row kind

// the books a byte holds: plain 1..256 values; pair rule: 1..255 normal values (255 is the identifier), 0..255 outliers
inline bool dec8_book_ok(int m, int n_normal, bool ovp)
{
    if (m < 1) return false;
    if (ovp) return n_normal >= 1 && n_normal <= 255 && m - n_normal >= 0 && m - n_normal <= 255;
    return m <= 256;
}

// One job's descriptor (d may be NULL) -> its number of tasks; ANTQ_ERR_* (< 0) when the job is refused.
inline long long dec8_job_tasks(const antq_decode_job &J, int dtype, unsigned flags, DecDesc *d)
{
    if (dtype != ANTQ_F32 && dtype != ANTQ_BF16 && dtype != ANTQ_F16) return ANTQ_ERR_UNSUPPORTED;
    if (!J.codes_dev || !J.out_dev || !J.alpha_dev || !J.grid_dev) return ANTQ_ERR_ARG;
    if (J.rows == 0 || J.row_len == 0) return ANTQ_ERR_ARG;
    if (J.row_len % 4 != 0) return ANTQ_ERR_UNSUPPORTED;
    if (J.m < 1) return ANTQ_ERR_ARG;
    if (!dec8_book_ok(J.m, J.n_normal, (flags & ANTQ_FLAG_OVP) != 0)) return ANTQ_ERR_UNSUPPORTED;
    if (J.rows > (size_t)-1 / J.row_len) return ANTQ_ERR_UNSUPPORTED;
    const size_t esz = dtype == ANTQ_F32 ? 4 : 2, epl = 16 / esz;
    if (reinterpret_cast<uintptr_t>(J.out_dev) % esz) return ANTQ_ERR_ALIGN;
    const size_t n = J.rows * J.row_len;
    const size_t rows = J.alpha_per_row ? J.rows : 1, row_len = J.alpha_per_row ? J.row_len : n;
    DecDesc D;
    memset(&D, 0, sizeof(D));
    size_t tasks;
    if (reinterpret_cast<uintptr_t>(J.codes_dev) % 4 || reinterpret_cast<uintptr_t>(J.out_dev) % 16 || row_len % epl != 0) {
        if (row_len / 4 > 0xffffffffull) return ANTQ_ERR_UNSUPPORTED;
        D.kind = kDec8Quad; D.n_units = n / 4; D.vpr = (uint32_t)(row_len / 4); D.tpr = 1; D.u = kDec8QuadU;
        tasks = (n / 4 + 64 * kDec8QuadU - 1) / (64 * kDec8QuadU);
    } else {
        const size_t vpr = row_len / epl;
        if (vpr > 0xffffffffull) return ANTQ_ERR_UNSUPPORTED;
        D.vpr = (uint32_t)vpr;
        if (vpr >= kDecRowMinVpr) {
            D.kind = kDec8Row;
            D.u = dec_row_u(D.vpr);
            const size_t span = 64u * D.u, tpr = (vpr + span - 1) / span;
            D.tpr = (uint32_t)tpr;
            if (rows > 0xfffffff0ull / tpr) return ANTQ_ERR_UNSUPPORTED;
            tasks = rows * tpr;
            D.rot = (vpr % span != 0 && tpr % 2 == 0) ? 1u : 0u;
        } else {
            D.kind = kDec8Lane; D.n_units = n / epl; D.tpr = 1; D.u = kDec8LaneU;
            tasks = (n / epl + 64 * kDec8LaneU - 1) / (64 * kDec8LaneU);
        }
    }
    if (tasks > 0x7ffffff0ull) return ANTQ_ERR_UNSUPPORTED;
    D.total_tasks = (uint32_t)tasks;
    D.codes = J.codes_dev; D.out = J.out_dev; D.alpha = J.alpha_dev; D.grid = J.grid_dev;
    D.m = (uint32_t)J.m; D.n_normal = (flags & ANTQ_FLAG_OVP) ? J.n_normal : 0; D.per_row = J.alpha_per_row ? 1 : 0; D.gmax = J.gmax;
    if (d) *d = D;
    return (long long)tasks;
}

inline size_t dec8_batch_capacity(const antq_decode_job *jobs, int n, int dtype) { return dec_blob_capacity(dec8_job_tasks, jobs, n, dtype); }
inline int dec8_batch_build(const antq_decode_job *jobs, int n, int dtype, unsigned flags, void *blob, size_t cap)
{
    return dec_blob_build(kDec8Magic, dec8_job_tasks, jobs, n, dtype, flags, blob, cap);
}

}  // namespace antq

#endif  // ANTQ_DECBATCH8_H
