// kernels_filter.hip -- row selection by bitmap: the chunk ordinals of a part,
// the gather list of a selective PREWHERE scan, the searched-chunk count of a
// row range, and the filter map of decoupled parts.
#include "flat_kernels.h"

namespace mqvs {

// Bitmap words: bits [32 w, 32 w + 32) of an LSB-first byte bitmap of nbits
// bits (bits at or past nbits read 0).  The row-selection kernels below work a
// word (32 rows) per lane and a wave per granule chunk: round 3's row-per-
// thread loops with a block barrier per 256 rows took 60-90 us each on a
// 50M-row part (6104 chunks), more than a 1 %-selective scan itself.
__device__ inline uint32_t bm_word(const uint8_t *bm, int64_t nbits, int64_t w) {
    const int64_t b0 = 4 * w, nbytes = (nbits + 7) >> 3;
    uint32_t v = 0;
    if (b0 + 4 <= nbytes && (((uintptr_t)(bm + b0)) & 3) == 0) {
        v = *reinterpret_cast<const uint32_t *>(bm + b0);
    } else {
        for (int i = 0; i < 4; ++i)
            if (b0 + i < nbytes) v |= (uint32_t)bm[b0 + i] << (8 * i);
    }
    const int64_t hi = nbits - 32 * w;
    if (hi < 32) v &= hi <= 0 ? 0u : ((1u << hi) - 1u);
    return v;
}

// rows of word w inside [r0, r1)
__device__ inline uint32_t range_mask(int64_t w, int64_t r0, int64_t r1) {
    const int64_t b = 32 * w;
    uint32_t m = 0xFFFFFFFFu;
    if (r0 > b) m = r0 - b >= 32 ? 0u : m & (0xFFFFFFFFu << (r0 - b));
    if (r1 < b + 32) m = r1 <= b ? 0u : m & ((1u << (r1 - b)) - 1u);
    return m;
}

// selected rows of word w: filter (or every row when null) & non-empty & live
__device__ inline uint32_t sel_word(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists,
                                    int64_t n, int64_t w) {
    uint32_t v = filter ? bm_word(filter, n, w) : range_mask(w, 0, n);
    if (nonempty) v &= bm_word(nonempty, n, w);
    if (exists) v &= bm_word(exists, n, w);
    return v;
}

__device__ inline int64_t wave_excl_scan64(int64_t v, int64_t &total) {
    const int lane = threadIdx.x & 63;
    int64_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    total = __shfl(inc, 63);
    return inc - v;
}

// Chunk ordinals: which granule chunks the reference actually hands to
// searchWrapper, and how many such calls came before each.
//  no-filter mode (require_filter = 0): a chunk is searched iff one of its
//    arrays is non-empty (MergeTreeVSManager.cpp:1364-1368 skips src_vec.empty());
//  filter mode: a mark is searched iff it keeps >= 1 selected non-empty live
//    row (:1179-1183).
// One wave per chunk, four chunks per workgroup.
__global__ __launch_bounds__(256) void k_chunk_active(const uint8_t *filter,
                                                       const uint8_t *nonempty,
                                                       const uint8_t *exists, int64_t n,
                                                       int64_t chunk_rows, int64_t nchunks, int require_filter,
                                                       int *flag) {
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const int64_t r0 = c * chunk_rows;
    const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
    uint32_t any = 0;
    for (int64_t w = (r0 >> 5) + lane; w < ((r1 + 31) >> 5) && !any; w += 64) {
        uint32_t v = range_mask(w, r0, r1);
        if (nonempty) v &= bm_word(nonempty, n, w);
        if (require_filter) {
            v &= bm_word(filter, n, w);
            if (exists) v &= bm_word(exists, n, w);
        }
        any |= v;
    }
    const bool hit = __any(any != 0);
    if (lane == 0) flag[c] = hit ? 1 : 0;
}

// One workgroup of kScanThreads: thread t owns a contiguous run of chunks;
// the run sums are scanned by waves, then over the wave totals.
constexpr int kScanThreads = 1024;
template <int NT = kScanThreads, class Val, class Out>
__device__ void run_scan(int64_t nchunks, Val val, Out out, int64_t *sh, int64_t &grand) {
    constexpr int kScanThreads = NT;  // block size of the caller
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t per = (nchunks + kScanThreads - 1) / kScanThreads;
    const int64_t b = t * per, e = b + per < nchunks ? b + per : nchunks;
    int64_t s = 0;
    for (int64_t i = b; i < e; ++i) s += val(i);
    int64_t wt = 0;
    const int64_t ex = wave_excl_scan64(s, wt);
    if (lane == 0) sh[wv] = wt;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) {
        if (w < wv) before += sh[w];
        all += sh[w];
    }
    int64_t run = before + ex;
    for (int64_t i = b; i < e; ++i) {
        const int64_t v = val(i);
        out(i, run, v);
        run += v;
    }
    grand = all;
    __syncthreads();
}

__global__ __launch_bounds__(kScanThreads) void k_exclusive_ord(int *flag_ord, int64_t nchunks) {
    __shared__ int64_t sh[kScanThreads / 64];
    int64_t tot = 0;
    run_scan(
        nchunks, [&](int64_t i) -> int64_t { return flag_ord[i] ? 1 : 0; },
        [&](int64_t i, int64_t before, int64_t v) { flag_ord[i] = v ? (int)before : -1; }, sh, tot);
}

void launch_chunk_ordinals(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists,
                           int64_t n, int64_t chunk_rows, int require_filter, int *ord,
                           hipStream_t s) {
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    if (nchunks < 1) return;
    hipLaunchKernelGGL(k_chunk_active, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, s, filter, nonempty,
                       exists, n, chunk_rows, nchunks, require_filter, ord);
    hipLaunchKernelGGL(k_exclusive_ord, dim3(1), dim3(kScanThreads), 0, s, ord, nchunks);
}

// ---------------------------------------------------------------------------
// Gather list of a selective PREWHERE scan: the rows that pass the filter,
// are non-empty and not deleted, chunk by chunk in row order, each chunk's
// run padded with -1 to a multiple of `tile` entries.
// k_chunk_count: per chunk its selected rows (one wave per chunk); the last
// workgroup to finish (an agent-scope ticket, zeroed with the search's status
// words) then scans the counts: offsets[c] = sum of padded counts before c,
// totals[0] = padded list length, totals[1] = selected rows.  host_totals
// (pinned host memory, may be null): the same two values, then host_gen in
// [2] behind a system-scope fence, so the host can act on them as soon as [2]
// shows its call's generation instead of draining the stream for a copy (a
// record left by another call's kernel never carries this call's number).
// (One launch: the separate single-workgroup scan cost ~8 us plus a launch
// gap.)
// The ticket relies on gfx9-family memory ordering (gfx950 here): stores with
// the agent-scope write-through and vmcnt counting stores, so a workgroup's
// counts have left it when its s_waitcnt vmcnt(0) (the 0x0F70 encoding: gfx9's
// field layout) retires, before its ticket; other ISA families order stores
// differently and would need release/acquire fences on the ticket.
constexpr int kCountStage = 16384;  // chunks whose counts k_chunk_count's scan stages in LDS

__global__ __launch_bounds__(kScanThreads) void k_chunk_count(const uint8_t *filter, const uint8_t *nonempty,
                                                               const uint8_t *exists, int64_t n, int64_t chunk_rows,
                                                               int64_t nchunks, int *count, int tile,
                                                               int64_t *offsets, int64_t *totals,
                                                               int64_t *host_totals, int64_t host_gen,
                                                               int *ticket) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "k_chunk_count's ticket assumes gfx94x/gfx950 store ordering (see above)"
#endif
    __shared__ int64_t sh[kScanThreads / 64];
    __shared__ int s_last;
    const int64_t c = (int64_t)blockIdx.x * (kScanThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c < nchunks) {
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        int cnt = 0;
        // (unrolled: a chunk of 8192 rows is 4 words per lane, their loads in
        // flight together)
#pragma unroll 4
        for (int64_t w = (r0 >> 5) + lane; w < ((r1 + 31) >> 5); w += 64)
            cnt += __popc(sel_word(filter, nonempty, exists, n, w) & range_mask(w, r0, r1));
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        // (write-through: the count reaches the device-coherent level
        // without an agent-scope release, which writes back the whole L2 --
        // one per workgroup cost ~50 us at 1526 workgroups)
        if (lane == 0) __hip_atomic_store(count + c, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // last workgroup in: every count stored and drained before the ticket
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();
    if (threadIdx.x == 0) {
        const int prev = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // (coherent loads of the other workgroups' counts, no acquire fence)
    // Up to kCountStage chunks: staged in LDS first, 8 independent loads in
    // flight per thread -- the two scans below read each count twice, and
    // reading them from memory there serialised ~18 coherent loads per thread
    // (k_chunk_count 21 us at 6104 chunks)
    extern __shared__ int s_cnt[];
    const bool staged = nchunks <= kCountStage;
    if (staged) {
        for (int64_t i0 = threadIdx.x; i0 < nchunks; i0 += 8 * kScanThreads) {
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t i = i0 + (int64_t)u * kScanThreads;
                v[u] = i < nchunks ? __hip_atomic_load(count + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t i = i0 + (int64_t)u * kScanThreads;
                if (i < nchunks) s_cnt[i] = v[u];
            }
        }
        __syncthreads();
    }
    auto cnt_of = [&](int64_t i) -> int64_t {
        if (staged) return (int64_t)s_cnt[i];
        return (int64_t)__hip_atomic_load(count + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    int64_t padded_total = 0, selected = 0;
    run_scan(
        nchunks, [&](int64_t i) -> int64_t { return (cnt_of(i) + tile - 1) / tile * tile; },
        [&](int64_t i, int64_t before, int64_t) { offsets[i] = before; }, sh, padded_total);
    run_scan(nchunks, cnt_of, [&](int64_t, int64_t, int64_t) {}, sh, selected);
    if (threadIdx.x == 0) {
        totals[0] = padded_total;
        totals[1] = selected;
        *ticket = 0;
        if (host_totals) {
            *reinterpret_cast<volatile int64_t *>(host_totals) = padded_total;
            *reinterpret_cast<volatile int64_t *>(host_totals + 1) = selected;
            __threadfence_system();
            *reinterpret_cast<volatile int64_t *>(host_totals + 2) = host_gen;
            __threadfence_system();
        }
    }
}

// one wave per chunk: lane l takes 4 consecutive words of each 256-word round,
// a wave scan of their counts places its rows
__global__ __launch_bounds__(256) void k_compact_rows(const uint8_t *filter, const uint8_t *nonempty,
                                                       const uint8_t *exists, int64_t n, int64_t chunk_rows,
                                                       int64_t nchunks, const int *count, const int64_t *offsets,
                                                       int tile, int32_t *list, int64_t list_end,
                                                       const int64_t *dev_total, int64_t round) {
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const int64_t r0 = c * chunk_rows;
    const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
    int32_t *out = list + offsets[c];
    int64_t run = 0;
    const int64_t w0 = r0 >> 5, w1 = (r1 + 31) >> 5;
    for (int64_t base = w0; base < w1; base += 256) {
        uint32_t v[4];
        int64_t cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t w = base + 4 * lane + i;
            v[i] = w < w1 ? sel_word(filter, nonempty, exists, n, w) & range_mask(w, r0, r1) : 0u;
            cnt += __popc(v[i]);
        }
        int64_t tot = 0;
        int64_t pos = run + wave_excl_scan64(cnt, tot);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t m = v[i];
            const int64_t rb = 32 * (base + 4 * lane + i);
            while (m) {
                const int bit = __ffs(m) - 1;
                m &= m - 1;
                out[pos++] = (int32_t)(rb + bit);
            }
        }
        run += tot;
    }
    const int cnt = count[c];
    const int padded = (cnt + tile - 1) / tile * tile;
    for (int i = cnt + lane; i < padded; i += 64) out[i] = -1;
    // the last chunk also pads the list's end up to list_end (whole tiles of
    // the scan; -1 entries); list_end < 0: the padded total k_chunk_count
    // left in device memory, rounded up to `round` (a list launched before
    // the host read the count)
    if (list_end < 0) list_end = (*dev_total + round - 1) / round * round;
    if (c == nchunks - 1)
        for (int64_t i = offsets[c] + padded + lane; i < list_end; i += 64) list[i] = -1;
}

void launch_gather_count(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists, int64_t n,
                         int64_t chunk_rows, int tile, int *count, int64_t *offsets, int64_t *totals,
                         int64_t *host_totals, int64_t host_gen, int *ticket, hipStream_t s) {
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    if (nchunks < 1) return;
    constexpr int wpb = kScanThreads / 64;  // chunks (waves) per workgroup
    const size_t lds = sizeof(int) * (size_t)(nchunks <= kCountStage ? nchunks : 0);
    hipLaunchKernelGGL(k_chunk_count, dim3((unsigned)((nchunks + wpb - 1) / wpb)), dim3(kScanThreads), lds, s, filter,
                       nonempty, exists, n, chunk_rows, nchunks, count, tile, offsets, totals, host_totals, host_gen,
                       ticket);
}

void launch_gather_list(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists, int64_t n,
                        int64_t chunk_rows, int tile, const int *count, const int64_t *offsets, int32_t *list,
                        int64_t list_end, hipStream_t s, const int64_t *dev_total, int64_t round) {
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    if (nchunks < 1) return;
    hipLaunchKernelGGL(k_compact_rows, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, s, filter, nonempty, exists,
                       n, chunk_rows, nchunks, count, offsets, tile, list, list_end, dev_total, round);
}

// ---------------------------------------------------------------------------
// searched chunks of a row range (the cosine chunk-ordinal base of the next
// shard): k_chunk_active flags, then one block sums them
__global__ __launch_bounds__(256) void k_sum_flags(const int *flags, int64_t nchunks, int64_t *count) {
    __shared__ int64_t part[256];
    int64_t s = 0;
    for (int64_t c = threadIdx.x; c < nchunks; c += 256) s += flags[c] ? 1 : 0;
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = part[0];
}

void launch_count_active_chunks(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists, int64_t n,
                                int64_t chunk_rows, int *flags_scratch, int64_t *count, hipStream_t s) {
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    if (nchunks > 0)
        hipLaunchKernelGGL(k_chunk_active, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, s, filter, nonempty,
                           exists, n, chunk_rows, nchunks, filter ? 1 : 0, flags_scratch);
    hipLaunchKernelGGL(k_sum_flags, dim3(1), dim3(256), 0, s, flags_scratch, nchunks, count);
}

// ---------------------------------------------------------------------------
// Decoupled parts (a merged part whose vector index still lives in its source
// parts): getRealBitmap (VIUtils.cpp:479-497) on the device (the id map of
// the results, transferToNewRowIds, is k_map_ids in kernels_util.hip).
__global__ void k_copy_bits(const uint8_t *src, int64_t rows, uint32_t *words) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w * 32 >= rows) return;
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b) {
        const int64_t byte = w * 4 + b;
        if (byte * 8 < rows) v |= (uint32_t)src[byte] << (8 * b);
    }
    const int64_t tail = rows - w * 32;
    if (tail < 32) v &= (1u << tail) - 1u;
    words[w] = v;
}

__global__ void k_decoupled_filter(const uint8_t *nf, int64_t new_rows, const uint64_t *inv_ids, const uint8_t *inv_src,
                                   int64_t inv_len, uint32_t own_id, uint32_t *old_words, int64_t old_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= new_rows || i >= inv_len) return;
    if (!((nf[i >> 3] >> (i & 7)) & 1)) return;
    if ((uint32_t)inv_src[i] != own_id) return;
    const uint64_t r = inv_ids[i];
    if (r < (uint64_t)old_rows) atomicOr(&old_words[r >> 5], 1u << (r & 31));
}

void launch_decoupled_filter(const uint8_t *new_filter, int64_t new_rows, const uint64_t *inv_ids,
                             const uint8_t *inv_src, int64_t inv_len, uint32_t own_id, uint32_t *old_words,
                             int64_t old_rows, hipStream_t s) {
    const int64_t nw = (old_rows + 31) / 32;
    MQVS_HIP(hipMemsetAsync(old_words, 0, 4 * (size_t)std::max<int64_t>(nw, 1), s));
    if (!inv_ids) {  // no maps: the filter itself ("return filter")
        if (nw) hipLaunchKernelGGL(k_copy_bits, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, new_filter,
                                   std::min(new_rows, old_rows), old_words);
        return;
    }
    if (new_rows > 0)
        hipLaunchKernelGGL(k_decoupled_filter, dim3((unsigned)((new_rows + 255) / 256)), dim3(256), 0, s, new_filter,
                           new_rows, inv_ids, inv_src, inv_len, own_id, old_words, old_rows);
}

}  // namespace mqvs
