// cand_list.h -- the per-query candidate list every APPEND scan writes and
// every select reads: cand[q][cap] records under count[q].
//
// The contract:
//   * Writers (the scan kernels, the probe selects) only append, through the
//     functions below.  Every taker bumps count[q], whether or not its record
//     fits, so count[q] is the number of takers, not of stored records.
//     Three scans keep their ballot and atomic in place and call cand_store
//     only -- emit_approx's per-query loop (scan_emit.h), k_scan_binary and
//     bivf_emit: behind cand_append_wave they compile to other instruction
//     streams (tools/diff_kernel_text.sh), and a hot kernel's schedule is not
//     worth a shared helper.
//   * A record whose slot is >= cap is dropped.  Slots [0, min(count, cap))
//     all hold records of this search, in no particular order.
//   * count[q] > cap is the only overflow signal.  A reader takes cand_len()
//     records (k_final_select writes the same two lines out), reports `over`, and must not make the list look whole again: a
//     kernel that rewrites an overflowed list keeps its count above cap
//     (k_refine copies it whole).  The host answers the flag by scanning the
//     part again: rescan_on_overflow, workspace.h.
//
// The list's fields come by reference and the functions are force-inlined, so
// a caller's p.cand / p.cand_count / p.cand_cap are read where they are used,
// as in the open-coded sequences these functions replaced.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mqvs {

// Candidate record: raw metric value (d for L2, ip for IP/cosine) + local row.
struct __attribute__((aligned(8))) Cand {
    float raw;
    uint32_t row;
};

// the bounds-checked store of a taker's record
__device__ __forceinline__ void cand_store(Cand *const &cand, const int &cap, int q, int slot, float raw,
                                           uint32_t row) {
    if (slot < cap) {
        Cand c;
        c.raw = raw;
        c.row = row;
        cand[(int64_t)q * cap + slot] = c;
    }
}

// one atomic per taker: rare appends spread over many queries
__device__ __forceinline__ void cand_append_one(Cand *const &cand, int *const &count, const int &cap, int q,
                                                float raw, uint32_t row) {
    cand_store(cand, cap, q, atomicAdd(&count[q], 1), raw, row);
}

// one atomic per wave: every active lane passes the same q, the lanes that
// take get consecutive slots
__device__ __forceinline__ void cand_append_wave(Cand *const &cand, int *const &count, const int &cap, int q,
                                                 bool take, float raw, uint32_t row) {
    const unsigned long long m = __ballot(take);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&count[q], __popcll(m));
    base = __shfl(base, leader);
    if (take) cand_store(cand, cap, q, base + __popcll(m & ((1ull << lane) - 1ull)), raw, row);
}

// the records a reader may take: min(count[q], cap); over = the list overflowed
__device__ __forceinline__ int cand_len(const int *count, int cap, int q, bool &over) {
    const int n = count[q];
    over = n > cap;
    return over ? cap : n;
}

}  // namespace mqvs
