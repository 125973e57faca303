// segment.hip -- segments: a data part's vector column resident in HBM.  The
// constructors (host rows, device rows, the generator, compressed column files,
// binary codes), what they prepare for the searches (norms, bitmaps, the bf16
// plane), the mqvs_segment_* entry points, and the two knn_*_raw functions,
// which search a segment of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "workspace.h"

namespace mqvs {

static std::atomic<int> g_prefilter{2};  // planes built by new segments (mqvs_set_prefilter)

static void prepare_segment(mqvs_segment *s, const uint8_t *dev_nonempty_bytes,
                            hipStream_t st) {
    if (dev_nonempty_bytes) {
        MQVS_HIP(hipMalloc((void **)&s->nonempty_bits, (size_t)(s->n + 7) / 8));
        s->bytes += (size_t)(s->n + 7) / 8;
        launch_pack_nonempty(dev_nonempty_bytes, s->n, s->nonempty_bits, st);
        const int64_t nchunks = (s->n + s->granule - 1) / s->granule;
        MQVS_HIP(hipMalloc((void **)&s->chunk_ord, sizeof(int) * std::max<int64_t>(nchunks, 1)));
        s->bytes += sizeof(int) * nchunks;
        launch_chunk_ordinals(nullptr, s->nonempty_bits, nullptr, s->n, s->granule, 0,
                              s->chunk_ord, st);
    }
    if (s->metric == MQVS_METRIC_COSINE) launch_normalize_rows(s->rows, s->n, s->d, st);
    // |y|^2 per row: the BLAS-branch L2 norms, and (all metrics) the bound of
    // the bf16 pre-filter
    MQVS_HIP(hipMalloc((void **)&s->norms, sizeof(float) * std::max<int64_t>(s->n, 1)));
    s->bytes += sizeof(float) * s->n;
    launch_row_norms(s->rows, s->n, s->d, s->norms, st);
    // bf16 plane of the rows for the nq >= 20 pre-filter (rows padded to kBfK)
    s->dpad = (s->d + kBfK - 1) / kBfK * kBfK;
    MQVS_HIP(hipMalloc((void **)&s->ynorm_max, 16 + sizeof(float) * kMxRec));
    MQVS_HIP(hipMemsetAsync(s->ynorm_max, 0, 16 + sizeof(float) * kMxRec, st));
    launch_max_norm(s->norms, s->n, s->ynorm_max, st);
    const int64_t nr = std::max<int64_t>(s->n, 1);
    const int64_t nr16 = (nr + 15) / 16 * 16;  // row-blocked planes: blocks of 16 rows
    const int split = g_prefilter.load(std::memory_order_relaxed);
    const size_t hb = (size_t)nr16 * s->dpad * sizeof(uint16_t);
    if (split == kHiSplit && hipMalloc((void **)&s->rows_hi, hb) == hipSuccess) {
        s->bytes += hb;
        launch_to_hi(s->rows, s->n, s->d, s->d, s->dpad, 1, nr16, s->rows_hi, nullptr, s->ynorm_max + 4, st);
        s->split = split;
        s->plane_bytes = hb;
    } else {
        (void)hipGetLastError();  // no room (or planes off): exact fp32 batch path only
        s->rows_hi = nullptr;
    }
    MQVS_HIP(hipGetLastError());
    float ymax = 0.f;
    MQVS_HIP(hipMemcpyAsync(&ymax, s->ynorm_max, sizeof(float), hipMemcpyDeviceToHost, st));
    MQVS_HIP(hipStreamSynchronize(st));
    // the bound needs finite, moderate norms (FLT_MAX-filled empty arrays of
    // L2/IP parts overflow): otherwise the exact fp32 path serves nq >= 20
    s->approx_ok = s->rows_hi != nullptr && ymax == ymax && ymax < 1e18f;
}

static void free_segment(mqvs_segment *s) {
    if (!s) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(s->device);
    if (s->rows_host)
        (void)hipHostFree(s->rows_host);
    else if (s->rows)
        (void)hipFree(s->rows);
    if (s->norms) (void)hipFree(s->norms);
    if (s->nonempty_bits) (void)hipFree(s->nonempty_bits);
    if (s->rows_hi) (void)hipFree(s->rows_hi);
    if (s->ynorm_max) (void)hipFree(s->ynorm_max);
    if (s->chunk_ord) (void)hipFree(s->chunk_ord);
    if (s->codes) (void)hipFree(s->codes);
    if (cur >= 0) (void)hipSetDevice(cur);
    delete s;
}

// A segment under construction, or a temporary one: freed with everything it
// holds unless released to the caller.
struct SegmentFree {
    void operator()(mqvs_segment *s) const { free_segment(s); }
};
using SegmentPtr = std::unique_ptr<mqvs_segment, SegmentFree>;

// What every constructor checks, in the order of its messages: the rows, the
// dimension and the metric (the caller's conditions and words), the granule,
// the row offset.
static void check_part_args(int64_t n, bool dim_ok, const char *dim_msg, bool metric_ok, const char *metric_msg,
                            int64_t granule, int64_t row_offset) {
    if (n < 0 || n >= ((int64_t)1 << 32)) fail(MQVS_ERR_BAD_ARGUMENTS, "segment rows must be in [0, 2^32)");
    if (!dim_ok) fail(MQVS_ERR_BAD_ARGUMENTS, dim_msg);
    if (!metric_ok) fail(MQVS_ERR_NOT_IMPLEMENTED, metric_msg);
    if (granule <= 0) fail(MQVS_ERR_BAD_ARGUMENTS, "granule_rows must be positive");
    if (row_offset < 0 || row_offset % granule != 0)
        fail(MQVS_ERR_BAD_ARGUMENTS, "row_offset must be a non-negative multiple of granule_rows");
}

static void check_seg_args(int64_t n, int32_t d, int32_t metric, int64_t granule,
                           int64_t row_offset) {
    check_part_args(n, d > 0, "dimension must be positive",
                    metric == MQVS_METRIC_L2 || metric == MQVS_METRIC_IP || metric == MQVS_METRIC_COSINE,
                    "Metric not implemented in brute force search for Float32 Vector", granule, row_offset);
}

// a segment of the current device with no memory yet
static SegmentPtr blank_segment(int64_t n, int32_t d, int32_t metric, int64_t granule, int64_t row_offset) {
    SegmentPtr s(new mqvs_segment());
    MQVS_HIP(hipGetDevice(&s->device));
    s->n = n;
    s->d = d;
    s->metric = metric;
    s->granule = granule;
    s->row_offset = row_offset;
    return s;
}

// its rows or codes: the first bytes it accounts for
static void alloc_payload(mqvs_segment &s, void **p, size_t bytes) {
    if (hipMalloc(p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of " + std::to_string(bytes) + " bytes failed");
    }
    s.bytes = bytes;
}

static SegmentPtr new_segment(int64_t n, int32_t d, int32_t metric, int64_t granule,
                              int64_t row_offset) {
    SegmentPtr s = blank_segment(n, d, metric, granule, row_offset);
    alloc_payload(*s, (void **)&s->rows, (size_t)std::max<int64_t>(n, 1) * d * sizeof(float));
    return s;
}

static SegmentPtr new_binary_segment(int64_t n, int32_t dim_bits, int32_t metric, int64_t granule,
                                     int64_t row_offset) {
    check_part_args(n, dim_bits > 0 && dim_bits % 8 == 0,
                    "binary vector dimension must be a positive multiple of 8 bits",
                    metric == MQVS_METRIC_HAMMING || metric == MQVS_METRIC_JACCARD,
                    "Metric not implemented in brute force search for Binary Vector", granule, row_offset);
    SegmentPtr s = blank_segment(n, dim_bits, metric, granule, row_offset);
    s->binary = true;
    s->code_bytes = dim_bits / 8;
    s->code_words = (int)round_up((s->code_bytes + 3) / 4, 4);
    alloc_payload(*s, (void **)&s->codes, (size_t)std::max<int64_t>(n, 1) * s->code_words * 4);
    return s;
}

// The constructors' entry: the handle must be there, and is null until the
// segment is whole.
static void open_handle(mqvs_segment_t *out) {
    if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
    *out = nullptr;
}

// The constructors' frame: a call on the workspace of the new segment's
// device, body(segment, workspace) filling the segment on that workspace's
// stream, the segment handed over.  A body that throws leaves *out null and
// the segment freed (after the call has ended).
template <typename Body>
static void build_segment(mqvs_segment_t *out, SegmentPtr s, Body &&body) {
    Workspace &ws = workspace(s->device);
    WsCall ws_call(ws);
    body(*s, ws);
    *out = s.release();
}

static bool all_nonempty(const uint8_t *ne, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!ne[i]) return false;
    return true;
}

// rows of `nbytes` (host or device) -> zero-padded [n][words] on the device
void upload_codes(uint32_t *dst, int words, const uint8_t *src, int64_t nbytes, int64_t n, bool dev,
                         hipStream_t s) {
    if (n <= 0) return;
    MQVS_HIP(hipMemsetAsync(dst, 0, (size_t)n * words * 4, s));
    MQVS_HIP(hipMemcpy2DAsync(dst, (size_t)words * 4, src, (size_t)nbytes, (size_t)nbytes, (size_t)n,
                              dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
}

// the result of a search over no rows: id -1 and the metric's worst distance
// (its bits: Hamming's is an int) in each of the m slots
static void fill_empty_result(int64_t m, int64_t *ids, float *dist, uint32_t worst_bits) {
    for (int64_t i = 0; i < m; ++i) {
        ids[i] = -1;
        std::memcpy(&dist[i], &worst_bits, sizeof(float));
    }
}

// ---------------------------------------------------------------------------
// column ingest: the compressed files of a part's Array(Float32) column,
// decoded in HBM (kernels_ingest.hip, kernels_lz4.hip, kernels_cityhash.hip)
// into the rows matrix + nonempty flags of
// MergeTreeVSManager.cpp:1381-1393, then prepared like any segment.

struct IngestTmp {
    std::vector<void *> bufs;
    void *alloc(size_t bytes) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) {
            (void)hipGetLastError();
            fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of " + std::to_string(bytes) + " bytes failed");
        }
        bufs.push_back(p);
        return p;
    }
    // side stream for the block checksums (overlaps the decode; joined before
    // the status is read)
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    ~IngestTmp() {
        if (side) (void)hipStreamSynchronize(side);
        for (void *p : bufs) (void)hipFree(p);
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        if (side) (void)hipStreamDestroy(side);
    }
};

constexpr int kBadDataChecksum = 8, kBadSizesChecksum = 16;  // status bits (decode uses 4)

// One compressed stream of the column on the device, and its block table
struct IngestStream {
    const uint8_t *src = nullptr;
    int64_t bytes = 0;
    IngestBlock *tab = nullptr;
    int64_t blocks = 0, out_bytes = 0;  // of the table: blocks, decompressed bytes
};

// One column's ingest into `seg` on stream s: the stages below, in this order.
struct ColumnIngest {
    mqvs_segment &seg;
    hipStream_t s;
    int64_t *h;  // pinned words of the workspace: the tables' and the scan's results, then the status
    IngestTmp tmp;
    IngestStream data, sizes;
    int *status = nullptr;     // device word both streams' kernels OR their verdicts into
    bool verify = false;       // block checksums on the side stream
    bool direct = false;       // every array has d elements: the data decodes straight into the rows
    uint64_t *dsizes = nullptr;
    float *ddata = nullptr;
    int64_t *offs = nullptr;

    ColumnIngest(mqvs_segment &sg, Workspace &ws)
        : seg(sg), s(ws.stream), h(reinterpret_cast<int64_t *>(ws.host_flags + 16)) {}

    // block table of one compressed stream
    void table(IngestStream &st, const char *what) {
        const int64_t maxb = st.bytes / 25 + 1;
        st.tab = (IngestBlock *)tmp.alloc(sizeof(IngestBlock) * (size_t)maxb);
        int64_t *dout = (int64_t *)tmp.alloc(4 * sizeof(int64_t));
        launch_block_table(st.src, st.bytes, st.tab, maxb, dout, s);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(h, dout, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        host_wait(s);
        if (h[2] == 2)
            fail(MQVS_ERR_NOT_IMPLEMENTED, std::string(what) + ": compression method other than LZ4 / NONE");
        if (h[2])
            fail(MQVS_ERR_ILLEGAL_COLUMN, std::string(what) + ": malformed compressed block chain (CANNOT_DECOMPRESS)");
        st.blocks = h[0];
        st.out_bytes = h[1];
    }

    // both streams where the kernels read them (host streams are copied), and their tables
    void stage_streams(const uint8_t *data_bin, int64_t data_bytes, const uint8_t *sizes_bin, int64_t sizes_bytes,
                       bool dev) {
        data.src = data_bin;
        data.bytes = data_bytes;
        sizes.src = sizes_bin;
        sizes.bytes = sizes_bytes;
        if (!dev) {
            auto *a = (uint8_t *)tmp.alloc((size_t)data_bytes);
            auto *b = (uint8_t *)tmp.alloc((size_t)sizes_bytes);
            if (data_bytes) MQVS_HIP(hipMemcpyAsync(a, data_bin, (size_t)data_bytes, hipMemcpyHostToDevice, s));
            if (sizes_bytes) MQVS_HIP(hipMemcpyAsync(b, sizes_bin, (size_t)sizes_bytes, hipMemcpyHostToDevice, s));
            data.src = a;
            sizes.src = b;
        }
        table(sizes, "array sizes stream");
        if (sizes.out_bytes != 8 * seg.n)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "array sizes stream holds " + std::to_string(sizes.out_bytes) +
                                              " bytes for " + std::to_string(seg.n) + " rows");
        table(data, "vector data stream");
        if (data.out_bytes % 4) fail(MQVS_ERR_ILLEGAL_COLUMN, "vector data stream is not a whole number of Float32");
    }

    // the status word, and the block checksums forked onto the side stream
    void fork_checksums(bool on) {
        status = (int *)tmp.alloc(sizeof(int) * 4);
        MQVS_HIP(hipMemsetAsync(status, 0, sizeof(int) * 4, s));
        verify = on;
        if (!verify) return;
        // CompressedReadBufferBase.cpp:192-196; the verdict is read before any decoded byte is used
        MQVS_HIP(hipStreamCreateWithFlags(&tmp.side, hipStreamNonBlocking));
        MQVS_HIP(hipEventCreateWithFlags(&tmp.fork, hipEventDisableTiming));
        MQVS_HIP(hipEventCreateWithFlags(&tmp.join, hipEventDisableTiming));
        MQVS_HIP(hipEventRecord(tmp.fork, s));
        MQVS_HIP(hipStreamWaitEvent(tmp.side, tmp.fork, 0));
        launch_block_checksum(sizes.src, sizes.tab, sizes.blocks, kBadSizesChecksum, status, nullptr, tmp.side);
        launch_block_checksum(data.src, data.tab, data.blocks, kBadDataChecksum, status, nullptr, tmp.side);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipEventRecord(tmp.join, tmp.side));
    }

    // both streams decoded and the sizes scanned; the scan's three words and
    // (after the checksums have joined) the status word read into h[0..3]
    void decode_and_scan() {
        const int64_t n = seg.n;
        dsizes = (uint64_t *)tmp.alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(n, 1));
        launch_decode_blocks(sizes.src, sizes.bytes, sizes.tab, sizes.blocks, (uint8_t *)dsizes, status, s);
        // the common case (every array has d elements) decodes straight into the rows
        direct = data.out_bytes == 4 * n * (int64_t)seg.d;
        ddata = direct ? seg.rows : (float *)tmp.alloc((size_t)data.out_bytes);
        launch_decode_blocks(data.src, data.bytes, data.tab, data.blocks, (uint8_t *)ddata, status, s);
        MQVS_HIP(hipGetLastError());
        const int64_t tiles = std::max<int64_t>(1, (n + 4095) / 4096);
        offs = (int64_t *)tmp.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1));
        auto *scratch = (int64_t *)tmp.alloc(sizeof(int64_t) * (size_t)tiles);
        auto *st = (int64_t *)tmp.alloc(sizeof(int64_t) * 4);
        MQVS_HIP(hipMemsetAsync(st, 0, sizeof(int64_t) * 4, s));
        if (n > 0) launch_sizes_scan(dsizes, n, seg.d, data.out_bytes / 4, offs, scratch, st, s);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(h, st, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (verify) MQVS_HIP(hipStreamWaitEvent(s, tmp.join, 0));
        MQVS_HIP(hipMemcpyAsync(h + 3, status, sizeof(int), hipMemcpyDeviceToHost, s));
        host_wait(s);
    }

    // what was read says about the column; returns the arrays that do not have d elements
    int64_t verdicts() const {
        const int hstatus = *reinterpret_cast<const int *>(h + 3);
        if (hstatus & (kBadSizesChecksum | kBadDataChecksum))
            fail(MQVS_ERR_CHECKSUM, std::string("Checksum doesn't match: corrupted data (") +
                                        (hstatus & kBadSizesChecksum ? "array sizes stream" : "vector data stream") +
                                        ", CityHash128 of a compressed block)");
        if (hstatus)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "malformed LZ4 block (CANNOT_DECOMPRESS)");
        const int64_t notd = h[0], nelem = h[1];
        if (h[2])  // (such sizes can sum to the right count modulo 2^64)
            fail(MQVS_ERR_ILLEGAL_COLUMN, std::to_string(h[2]) + " array sizes exceed the " +
                                              std::to_string(data.out_bytes / 4) + " elements of the data stream");
        if (nelem * 4 != data.out_bytes)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "array sizes sum to " + std::to_string(nelem) + " elements, the data stream "
                                              "holds " + std::to_string(data.out_bytes / 4));
        return notd;
    }

    // ragged or empty arrays: the reference's copy loop; returns the nonempty flags it wrote
    const uint8_t *copy_ragged() {
        const float *srcdata = ddata;
        if (direct) {
            auto *copy = (float *)tmp.alloc((size_t)data.out_bytes);
            MQVS_HIP(hipMemcpyAsync(copy, ddata, (size_t)data.out_bytes, hipMemcpyDeviceToDevice, s));
            srcdata = copy;
        }
        auto *ne = (uint8_t *)tmp.alloc((size_t)std::max<int64_t>(seg.n, 1));
        launch_array_rows(srcdata, offs, dsizes, seg.n, seg.d, seg.rows, ne, s);
        MQVS_HIP(hipGetLastError());
        return ne;
    }
};

static void ingest_column(const uint8_t *data_bin, int64_t data_bytes, const uint8_t *sizes_bin, int64_t sizes_bytes,
                          int64_t n, int32_t d, int32_t metric, int64_t granule, int64_t row_offset, uint32_t flags,
                          mqvs_segment_t *out) {
    check_seg_args(n, d, metric, granule, row_offset);
    if (data_bytes < 0 || sizes_bytes < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "negative stream size");
    if ((data_bytes > 0 && !data_bin) || (sizes_bytes > 0 && !sizes_bin))
        fail(MQVS_ERR_BAD_ARGUMENTS, "null column stream");
    build_segment(out, new_segment(n, d, metric, granule, row_offset), [&](mqvs_segment &seg, Workspace &ws) {
        ColumnIngest in(seg, ws);
        in.stage_streams(data_bin, data_bytes, sizes_bin, sizes_bytes, (flags & MQVS_F_DEVICE_PTRS) != 0);
        in.fork_checksums(!(flags & MQVS_F_NO_CHECKSUM));
        in.decode_and_scan();
        const int64_t notd = in.verdicts();
        const uint8_t *nonempty = in.direct && notd == 0 ? nullptr : in.copy_ragged();
        prepare_segment(&seg, nonempty, in.s);  // synchronises the stream
    });
}

// ---------------------------------------------------------------------------
// services for the index path (index.hip)

mqvs_segment *segment_from_device(const float *dev_rows, int64_t n, int d, int metric, hipStream_t st) {
    SegmentPtr s = new_segment(n, d, metric, std::max<int64_t>(n, 1), 0);
    if (n > 0)
        MQVS_HIP(hipMemcpyAsync(s->rows, dev_rows, sizeof(float) * (size_t)n * d, hipMemcpyDeviceToDevice, st));
    prepare_segment(s.get(), nullptr, st);
    return s.release();
}

void segment_release(mqvs_segment *s) { free_segment(s); }

}  // namespace mqvs

using namespace mqvs;

// ---------------------------------------------------------------------------
extern "C" {

int mqvs_set_prefilter(int split) {
    if (split != kHiSplit && split != 0) return MQVS_ERR_BAD_ARGUMENTS;
    g_prefilter.store(split);
    return MQVS_OK;
}

int mqvs_segment_create(const float *host_rows, int64_t n, int32_t d, int32_t metric,
                        int64_t granule_rows, const uint8_t *nonempty, int64_t row_offset,
                        mqvs_segment_t *out) {
    return guarded([&] {
        open_handle(out);
        check_seg_args(n, d, metric, granule_rows, row_offset);
        if (n > 0 && !host_rows) fail(MQVS_ERR_BAD_ARGUMENTS, "null rows");
        build_segment(out, new_segment(n, d, metric, granule_rows, row_offset), [&](mqvs_segment &s, Workspace &ws) {
            if (n > 0)
                MQVS_HIP(hipMemcpyAsync(s.rows, host_rows, sizeof(float) * (size_t)n * d,
                                        hipMemcpyHostToDevice, ws.stream));
            const uint8_t *dne = nullptr;
            if (nonempty && n > 0 && !all_nonempty(nonempty, n)) {
                auto *b = (uint8_t *)ws.misc.get((size_t)n);
                MQVS_HIP(hipMemcpyAsync(b, nonempty, (size_t)n, hipMemcpyHostToDevice, ws.stream));
                dne = b;
            }
            prepare_segment(&s, dne, ws.stream);
        });
    });
}

int mqvs_segment_create_device(const float *dev_rows, int64_t n, int32_t d, int32_t metric,
                               int64_t granule_rows, const uint8_t *dev_nonempty,
                               int64_t row_offset, mqvs_segment_t *out) {
    return guarded([&] {
        open_handle(out);
        check_seg_args(n, d, metric, granule_rows, row_offset);
        if (n > 0 && !dev_rows) fail(MQVS_ERR_BAD_ARGUMENTS, "null rows");
        build_segment(out, new_segment(n, d, metric, granule_rows, row_offset), [&](mqvs_segment &s, Workspace &ws) {
            if (n > 0)
                MQVS_HIP(hipMemcpyAsync(s.rows, dev_rows, sizeof(float) * (size_t)n * d,
                                        hipMemcpyDeviceToDevice, ws.stream));
            prepare_segment(&s, dev_nonempty, ws.stream);
        });
    });
}

int mqvs_segment_generate(uint64_t seed, int32_t mode, int64_t n, int32_t d, int32_t metric,
                          int64_t granule_rows, int64_t row_offset, mqvs_segment_t *out) {
    return guarded([&] {
        open_handle(out);
        check_seg_args(n, d, metric, granule_rows, row_offset);
        if (mode < 0 || mode > 3) fail(MQVS_ERR_BAD_ARGUMENTS, "generator mode must be 0, 1, 2 or 3");
        build_segment(out, new_segment(n, d, metric, granule_rows, row_offset), [&](mqvs_segment &s, Workspace &ws) {
            launch_generate(seed, mode, row_offset, n, d, s.rows, ws.stream);
            MQVS_HIP(hipGetLastError());
            prepare_segment(&s, nullptr, ws.stream);
        });
    });
}

int mqvs_segment_create_from_column(const uint8_t *data_bin, int64_t data_bytes, const uint8_t *sizes_bin,
                                    int64_t sizes_bytes, int64_t n, int32_t d, int32_t metric, int64_t granule_rows,
                                    int64_t row_offset, uint32_t flags, mqvs_segment_t *out) {
    return guarded([&] {
        open_handle(out);
        ingest_column(data_bin, data_bytes, sizes_bin, sizes_bytes, n, d, metric, granule_rows, row_offset, flags,
                      out);
    });
}

int mqvs_segment_create_binary(const uint8_t *codes, int64_t n, int32_t dim_bits, int32_t metric,
                               int64_t granule_rows, int64_t row_offset, uint32_t flags, mqvs_segment_t *out) {
    return guarded([&] {
        open_handle(out);
        SegmentPtr seg = new_binary_segment(n, dim_bits, metric, granule_rows, row_offset);
        if (n > 0 && !codes) fail(MQVS_ERR_BAD_ARGUMENTS, "null codes");
        build_segment(out, std::move(seg), [&](mqvs_segment &s, Workspace &ws) {
            upload_codes(s.codes, s.code_words, codes, s.code_bytes, n, (flags & MQVS_F_DEVICE_PTRS) != 0,
                         ws.stream);
            MQVS_HIP(hipStreamSynchronize(ws.stream));
        });
    });
}

int mqvs_segment_free(mqvs_segment_t seg) {
    return guarded([&] { free_segment(seg); });
}

int mqvs_segment_info(mqvs_segment_t seg, int64_t *n, int32_t *d, int32_t *metric,
                      int64_t *granule_rows, int64_t *row_offset, size_t *hbm_bytes) {
    return guarded([&] {
        if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
        if (n) *n = seg->n;
        if (d) *d = seg->d;
        if (metric) *metric = seg->metric;
        if (granule_rows) *granule_rows = seg->granule;
        if (row_offset) *row_offset = seg->row_offset;
        if (hbm_bytes) *hbm_bytes = seg->bytes;
    });
}

int mqvs_segment_prefilter(mqvs_segment_t seg, int32_t *split, size_t *plane_bytes, int32_t *approx_ok) {
    return guarded([&] {
        if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
        const bool planes = !seg->binary && seg->rows_hi != nullptr;
        if (split) *split = planes ? seg->split : 0;
        if (plane_bytes) *plane_bytes = planes ? seg->plane_bytes : 0;
        if (approx_ok) *approx_ok = !seg->binary && seg->approx_ok ? 1 : 0;
    });
}

int mqvs_segment_set_rows_host(mqvs_segment_t seg, int32_t host) {
    return guarded([&] {
        if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
        if (seg->binary) fail(MQVS_ERR_LOGICAL, "binary segment has no Float32 rows");
        if ((host != 0) == (seg->rows_host != nullptr)) return;
        DeviceGuard guard(seg->device);
        const size_t bytes = sizeof(float) * (size_t)std::max<int64_t>(seg->n, 1) * (size_t)seg->d;
        MQVS_HIP(hipDeviceSynchronize());  // (work queued on the rows, e.g. by the segment's creation)
        if (host) {
            void *h = nullptr;
            if (hipHostMalloc(&h, bytes, hipHostMallocMapped) != hipSuccess)
                fail(MQVS_ERR_MEMORY_LIMIT, "pinned host memory for the rows (" + std::to_string(bytes) + " bytes)");
            void *dptr = nullptr;
            const hipError_t e1 = hipMemcpy(h, seg->rows, bytes, hipMemcpyDeviceToHost);
            const hipError_t e2 = e1 == hipSuccess ? hipHostGetDevicePointer(&dptr, h, 0) : e1;
            if (e2 != hipSuccess) {
                (void)hipHostFree(h);
                MQVS_HIP(e2);
            }
            (void)hipFree(seg->rows);
            seg->rows = static_cast<float *>(dptr);
            seg->rows_host = h;
            seg->bytes -= std::min(seg->bytes, bytes);
        } else {
            float *d = nullptr;
            if (hipMalloc((void **)&d, bytes) != hipSuccess)
                fail(MQVS_ERR_MEMORY_LIMIT, "HBM for the rows (" + std::to_string(bytes) + " bytes)");
            const hipError_t e = hipMemcpy(d, seg->rows_host, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(d);
                MQVS_HIP(e);
            }
            (void)hipHostFree(seg->rows_host);
            seg->rows_host = nullptr;
            seg->rows = d;
            seg->bytes += bytes;
        }
    });
}

int mqvs_segment_rows_host(mqvs_segment_t seg, int32_t *host) {
    return guarded([&] {
        if (!seg || !host) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        *host = seg->rows_host != nullptr ? 1 : 0;
    });
}

int mqvs_segment_rows(mqvs_segment_t seg, const float **dev_rows) {
    return guarded([&] {
        if (!seg || !dev_rows) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (seg->binary) fail(MQVS_ERR_LOGICAL, "binary segment has no Float32 rows");
        *dev_rows = seg->rows;
    });
}

int mqvs_knn_raw(const float *x, const float *y, int64_t d, int64_t k, int64_t nx, int64_t ny,
                 int32_t metric, int64_t *result_id, float *distance) {
    return guarded([&] {
        if (metric != MQVS_METRIC_L2 && metric != MQVS_METRIC_IP)
            fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Float32 Vector");
        fault_point();
        if (d <= 0 || d > INT32_MAX || k < 0 || k > INT32_MAX || nx < 0 || nx > INT32_MAX || ny < 0)
            fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if (nx == 0 || k == 0) return;
        if (ny == 0) {
            const float worst = metric == MQVS_METRIC_L2 ? 3.40282347e+38f : -3.40282347e+38f;
            fill_empty_result(nx * k, result_id, distance, __builtin_bit_cast(uint32_t, worst));
            return;
        }
        SegmentPtr s = new_segment(ny, (int)d, metric, ny, 0);
        Workspace &ws = workspace(s->device);
        WsCall ws_call(ws);
        MQVS_HIP(hipMemcpyAsync(s->rows, y, sizeof(float) * (size_t)ny * d, hipMemcpyHostToDevice,
                                ws.stream));
        prepare_segment(s.get(), nullptr, ws.stream);
        search_internal(s.get(), x, (int)nx, (int)k, metric == MQVS_METRIC_IP ? kMetricIpRaw : MQVS_METRIC_L2,
                        nullptr, nullptr, result_id, distance, 0, nullptr);
    });
}

int mqvs_knn_binary_raw(const uint8_t *x, const uint8_t *y, int64_t d, int64_t k, int64_t nx, int64_t ny,
                        int32_t metric, int64_t *result_id, float *distance) {
    return guarded([&] {
        if (metric != MQVS_METRIC_HAMMING && metric != MQVS_METRIC_JACCARD)
            fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Binary Vector");
        fault_point();
        if (d <= 0 || d % 8 != 0 || d > INT32_MAX || k < 0 || k > INT32_MAX || nx < 0 || nx > INT32_MAX ||
            ny < 0)
            fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if (nx == 0 || k == 0) return;
        if (ny == 0) {
            // (Hamming distances are int32 counts in the float array)
            fill_empty_result(nx * k, result_id, distance,
                              metric == MQVS_METRIC_HAMMING ? (uint32_t)INT32_MAX
                                                            : __builtin_bit_cast(uint32_t, 3.40282347e+38f));
            return;
        }
        SegmentPtr s = new_binary_segment(ny, (int32_t)d, metric, ny, 0);
        Workspace &ws = workspace(s->device);
        WsCall ws_call(ws);
        upload_codes(s->codes, s->code_words, y, s->code_bytes, ny, false, ws.stream);
        const size_t m = (size_t)nx * k;
        auto *b = (char *)ws.misc.get(m * 12 + 16);
        auto *di = (int64_t *)b;
        auto *dd = (float *)(b + m * 8);
        auto *qd = (uint8_t *)ws.glist.get((size_t)nx * (d / 8));
        MQVS_HIP(hipMemcpyAsync(qd, x, (size_t)nx * (d / 8), hipMemcpyHostToDevice, ws.stream));
        search_binary(s.get(), qd, (int)nx, (int)k, metric, nullptr, nullptr, di, dd, MQVS_F_DEVICE_PTRS,
                           nullptr);
        if (metric == MQVS_METRIC_HAMMING) launch_hamming_to_int(di, dd, (int64_t)m, ws.stream);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(result_id, di, m * 8, hipMemcpyDeviceToHost, ws.stream));
        MQVS_HIP(hipMemcpyAsync(distance, dd, m * 4, hipMemcpyDeviceToHost, ws.stream));
        MQVS_HIP(hipStreamSynchronize(ws.stream));
    });
}

}  // extern "C"
