// antq_decbatch.h -- the batched packed-4-bit decoder's descriptor blob and its pure-host builder
// (antq_decode4_batch_capacity / antq_decode4_batch_build).  No HIP in this file: antq_plan.cpp compiles the builder, the
// kernel (antq_k_decbatch.h) reads the same structs.
//
// blob:  DecHeader | DecDesc descs[n] | uint32 map[total_blocks]
// A map entry stands for 4 consecutive tasks of one job (4 one-wavefront workgroups), as in the fake-quant batch
// (antq_k_batch.h: family 5); a task never leaves its job.  Task kinds:
//   kDecRow   rows of >= 128 output vectors (and every per-tensor-scale job that long): a task is u x 64 vectors inside ONE
//             row, so one scale -- the wavefront builds a 256-entry table keyed by the code BYTE (both outputs of the pair,
//             the pair rule included) and every pair costs one LDS read
//   kDecLane  shorter rows: u x 64 vectors of the flat tensor, the scale per lane (a vector never leaves its row:
//             row_len % 8 == 0), 16-entry codebook in LDS
//   kDecElem  codes not 4-byte or out not 16-byte aligned: 64 x 4 octets per task, byte loads and element stores
#ifndef ANTQ_DECBATCH_H
#define ANTQ_DECBATCH_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/antq.h"

namespace antq {

constexpr uint32_t kDecMagic = 0x34444E41u;    // "AND4"
constexpr uint32_t kDecRow = 0, kDecLane = 1, kDecElem = 2;
constexpr uint32_t kDecRowMinVpr = 128;        // rows from here amortise the 256-entry table (4 entries per lane)
constexpr uint32_t kDecElemU = 4;              // octets per lane and task of the element-granular kind

struct DecDesc {   // 88 bytes, device-visible
    const uint8_t *codes;
    void *out;
    const float *alpha;
    const float *grid;
    uint64_t n_units;      // kDecLane: 16-byte output vectors of the job; kDecElem: octets
    uint32_t total_tasks;
    uint32_t vpr;          // vectors per row (kDecRow: per-tensor scale = the whole tensor); kDecElem: octets per row
    uint32_t tpr;          // kDecRow: tasks per row
    uint32_t first_block;  // first map entry of this job
    uint32_t kind;
    uint32_t u;            // vectors per lane and task (kDecRow: 2 / 3 / 4)
    uint32_t rot;          // kDecRow: rotate the workgroup -> task map per group of 8 (partial last tasks would line up with
                           // the XCD number otherwise: antq_k_batch.h)
    uint32_t m;
    int32_t n_normal;
    int32_t per_row;
    float gmax;
    uint32_t pad_;
};
static_assert(sizeof(DecDesc) == 88, "DecDesc must be 88 bytes");

struct DecHeader {   // 32 bytes
    uint32_t magic, n, dtype, flags, map_offset, bytes, total_blocks, pad_;
};
static_assert(sizeof(DecHeader) == 32, "DecHeader must be 32 bytes");

// vectors per lane of a row task: the u in {4, 3, 2} with the fewest idle lanes (ties: the larger, the table is built once per task)
inline uint32_t dec_row_u(uint32_t vpr)
{
    uint32_t best_u = 4;
    double best = -1.0;
    for (uint32_t u = 4; u >= 2; u--) {
        const uint32_t span = 64u * u, tasks = (vpr + span - 1u) / span;
        const double util = (double)vpr / (double)tasks / (double)span;
        if (util > best + 1e-9) { best = util; best_u = u; }
    }
    return best_u;
}

// the books a nibble holds: plain 1..16 values; pair rule: 1..15 normal values (15 is the identifier), 0..15 outliers
inline bool dec4_book_ok(int m, int n_normal, bool ovp)
{
    if (ovp) return n_normal >= 1 && n_normal <= 15 && m - n_normal >= 0 && m - n_normal <= 15;
    return m <= 16;
}

// One job's descriptor (d may be NULL) -> its number of tasks; ANTQ_ERR_* (< 0) when the job is refused.
inline long long dec_job_tasks(const antq_decode_job &J, int dtype, unsigned flags, DecDesc *d)
{
    if (dtype != ANTQ_F32 && dtype != ANTQ_BF16 && dtype != ANTQ_F16) return ANTQ_ERR_UNSUPPORTED;
    if (!J.codes_dev || !J.out_dev || !J.alpha_dev || !J.grid_dev) return ANTQ_ERR_ARG;
    if (J.rows == 0 || J.row_len == 0) return ANTQ_ERR_ARG;
    if (J.row_len % 8 != 0) return ANTQ_ERR_UNSUPPORTED;
    if (J.m < 1) return ANTQ_ERR_ARG;
    if (!dec4_book_ok(J.m, J.n_normal, (flags & ANTQ_FLAG_OVP) != 0)) return ANTQ_ERR_UNSUPPORTED;
    if (J.rows > (size_t)-1 / J.row_len) return ANTQ_ERR_UNSUPPORTED;
    const size_t esz = dtype == ANTQ_F32 ? 4 : 2, epl = 16 / esz;
    if (reinterpret_cast<uintptr_t>(J.out_dev) % esz) return ANTQ_ERR_ALIGN;
    const size_t n = J.rows * J.row_len;
    const size_t rows = J.alpha_per_row ? J.rows : 1, row_len = J.alpha_per_row ? J.row_len : n;
    DecDesc D;
    memset(&D, 0, sizeof(D));
    size_t tasks;
    if (reinterpret_cast<uintptr_t>(J.codes_dev) % 4 || reinterpret_cast<uintptr_t>(J.out_dev) % 16) {
        if (row_len / 8 > 0xffffffffull) return ANTQ_ERR_UNSUPPORTED;
        D.kind = kDecElem; D.n_units = n / 8; D.vpr = (uint32_t)(row_len / 8); D.tpr = 1; D.u = kDecElemU;
        tasks = (n / 8 + 64 * kDecElemU - 1) / (64 * kDecElemU);
    } else {
        const size_t vpr = row_len / epl;
        if (vpr > 0xffffffffull) return ANTQ_ERR_UNSUPPORTED;
        D.vpr = (uint32_t)vpr;
        if (vpr >= kDecRowMinVpr) {
            D.kind = kDecRow;
            D.u = dec_row_u(D.vpr);
            const size_t span = 64u * D.u, tpr = (vpr + span - 1) / span;
            D.tpr = (uint32_t)tpr;
            if (rows > 0xfffffff0ull / tpr) return ANTQ_ERR_UNSUPPORTED;
            tasks = rows * tpr;
            D.rot = (vpr % span != 0 && tpr % 2 == 0) ? 1u : 0u;
        } else {
            D.kind = kDecLane; D.n_units = n / epl; D.tpr = 1; D.u = 4;
            tasks = (n / epl + 255) / 256;
        }
    }
    if (tasks > 0xfffffff0ull) return ANTQ_ERR_UNSUPPORTED;
    D.total_tasks = (uint32_t)tasks;
    D.codes = J.codes_dev; D.out = J.out_dev; D.alpha = J.alpha_dev; D.grid = J.grid_dev;
    D.m = (uint32_t)J.m; D.n_normal = (flags & ANTQ_FLAG_OVP) ? J.n_normal : 0; D.per_row = J.alpha_per_row ? 1 : 0; D.gmax = J.gmax;
    if (d) *d = D;
    return (long long)tasks;
}

// The blob's builder, written once for both code widths: `job_tasks` is dec_job_tasks or dec8_job_tasks (antq_decbatch8.h),
// `magic` the blob's.
typedef long long (*dec_job_tasks_fn)(const antq_decode_job &, int, unsigned, DecDesc *);

inline size_t dec_blob_capacity(dec_job_tasks_fn job_tasks, const antq_decode_job *jobs, int n, int dtype)
{
    if (!jobs || n < 1 || n > 65535) return 0;
    size_t blocks = 0;
    for (int i = 0; i < n; i++) {
        // (the codebook changes no task count, and the flags are not known here; a job the builder will refuse counts as empty)
        antq_decode_job J = jobs[i];
        J.m = 1;
        const long long t = job_tasks(J, dtype, 0u, nullptr);
        if (t > 0) blocks += ((size_t)t + 3) / 4;
    }
    return sizeof(DecHeader) + sizeof(DecDesc) * (size_t)n + 4 * blocks;
}

inline int dec_blob_build(uint32_t magic, dec_job_tasks_fn job_tasks, const antq_decode_job *jobs, int n, int dtype, unsigned flags,
                          void *blob, size_t cap)
{
    if (!jobs || !blob || n < 1 || n > 65535) return ANTQ_ERR_ARG;
    if (flags & ~ANTQ_FLAG_OVP) return ANTQ_ERR_ARG;
    DecHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = magic; h.n = (uint32_t)n; h.dtype = (uint32_t)dtype; h.flags = flags;
    h.map_offset = (uint32_t)(sizeof(DecHeader) + sizeof(DecDesc) * (size_t)n);
    // every refusal first: nothing is written for a batch that cannot run
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        const long long t = job_tasks(jobs[i], dtype, flags, nullptr);
        if (t < 0) return (int)t;
        total += ((size_t)t + 3) / 4;
    }
    if (total > 0x1fffffffull) return ANTQ_ERR_UNSUPPORTED;       // (x 4 one-wavefront workgroups in one grid)
    const size_t bytes = h.map_offset + 4 * total;
    if (bytes > 0x7fffffffull) return ANTQ_ERR_UNSUPPORTED;
    if (cap < bytes) return ANTQ_ERR_PLAN;
    char *p = static_cast<char *>(blob);
    uint32_t first = 0;
    for (int i = 0; i < n; i++) {
        DecDesc D;
        const size_t nb = ((size_t)job_tasks(jobs[i], dtype, flags, &D) + 3) / 4;
        D.first_block = first;
        memcpy(p + sizeof(DecHeader) + sizeof(DecDesc) * (size_t)i, &D, sizeof(D));
        for (size_t b = 0; b < nb; b++) {
            const uint32_t job = (uint32_t)i;
            memcpy(p + h.map_offset + 4 * ((size_t)first + b), &job, 4);
        }
        first += (uint32_t)nb;
    }
    h.total_blocks = (uint32_t)total;
    h.bytes = (uint32_t)bytes;
    memcpy(p, &h, sizeof(h));
    return (int)h.bytes;
}

inline size_t dec_batch_capacity(const antq_decode_job *jobs, int n, int dtype) { return dec_blob_capacity(dec_job_tasks, jobs, n, dtype); }
inline int dec_batch_build(const antq_decode_job *jobs, int n, int dtype, unsigned flags, void *blob, size_t cap)
{
    return dec_blob_build(kDecMagic, dec_job_tasks, jobs, n, dtype, flags, blob, cap);
}

}  // namespace antq

#endif  // ANTQ_DECBATCH_H
