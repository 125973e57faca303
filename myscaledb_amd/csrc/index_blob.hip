// index_blob.hip -- index persistence of libmqvs: mqvs_index_save,
// mqvs_index_load, mqvs_index_blob_info (the index itself: index.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "index_internal.h"

namespace mqvs {

// ---- persistence: mqvs_index_save / mqvs_index_load -------------------------
// A saved index is the five things a build decides -- centroids, each row's
// list, nlist, alpha, np95 -- behind a 64-byte header, framed as a ClickHouse
// CompressedWriteBuffer stream (include/mqvs.h has the layout byte by byte).
// Everything else is derived again by finish_index.  The framing reuses the
// column ingest's device code in both directions: launch_block_table
// (kernels_ingest.hip) and launch_decode_blocks (kernels_lz4.hip) read it,
// launch_block_checksum (kernels_cityhash.hip) verifies it and, through
// hash_out, computes the checksums the writer stores.

constexpr int64_t kBlobBlock = 1 << 20;  // payload bytes of the blocks mqvs_index_save writes
constexpr int64_t kBlobFrame = 25;       // 16-B checksum + method byte + two UInt32 sizes
constexpr char kBlobMagic[8] = {'M', 'Q', 'V', 'S', 'I', 'D', 'X', '\0'};
constexpr int kFingerprintRows = 1024;

struct BlobHeader {  // little-endian, as the host is
    char magic[8];
    uint32_t version, kind, metric, dim;
    uint64_t n, nlist;
    uint32_t alpha_bits, np95;
    uint64_t fingerprint;
    uint32_t plane_fmt;  // MQVS_INDEX_PLANE_* (zero on a binary index)
    uint8_t reserved[4];
};
static_assert(sizeof(BlobHeader) == MQVS_INDEX_BLOB_HEADER_BYTES, "the documented header");

static void put_block_header(uint8_t *h, uint32_t payload) {  // h: the 9 bytes after the checksum
    const uint32_t csize = payload + 9;
    h[0] = 0x02;
    for (int i = 0; i < 4; ++i) {
        h[1 + i] = (uint8_t)(csize >> (8 * i));
        h[5 + i] = (uint8_t)(payload >> (8 * i));
    }
}

static int64_t row_bytes_of(const mqvs_segment *seg) { return seg->binary ? seg->code_bytes : 4 * (int64_t)seg->d; }

// The fingerprint of a segment's resident rows: S = min(n, 1024) rows, row
// floor(i n / S) for i < S (the builds' sample rule), gathered back to back (a
// float row as its d fp32 values as they are resident -- normalised for a
// cosine segment --, a binary row as its dim_bits / 8 code bytes) and framed as
// the payload of one method-NONE block; the fingerprint is the low 64 bits of
// that block's CityHash128 checksum (k_block_checksum, one lane).  The rows are
// read through seg->rows / seg->codes, which for rows moved to host memory is
// the mapped address of the pinned copy.
static uint64_t segment_fingerprint(mqvs_segment *seg, hipStream_t s) {
    const int64_t n = seg->n, S = std::min<int64_t>(n, kFingerprintRows), rb = row_bytes_of(seg);
    const int64_t len = S * rb;
    // the block starts at byte 7, so that its payload starts at byte 32
    TmpBuf buf(32 + (size_t)len + 16), tab(sizeof(IngestBlock)), out(sizeof(uint64_t) * 2 + sizeof(int) * 2);
    uint8_t pre[32] = {};
    put_block_header(pre + 23, (uint32_t)len);
    IngestBlock b{};
    b.src = 32;
    b.csize = b.usize = (uint32_t)len;
    b.method = 0x02;
    MQVS_HIP(hipMemcpyAsync(buf.p, pre, 32, hipMemcpyHostToDevice, s));
    MQVS_HIP(hipMemcpyAsync(tab.p, &b, sizeof(b), hipMemcpyHostToDevice, s));
    MQVS_HIP(hipMemsetAsync(out.p, 0, sizeof(uint64_t) * 2 + sizeof(int) * 2, s));
    std::vector<int64_t> idx64(S);
    std::vector<int32_t> idx32(S);
    for (int64_t i = 0; i < S; ++i) idx32[i] = (int32_t)(idx64[i] = (int64_t)((__int128)i * n / S));
    TmpBuf didx(sizeof(int64_t) * std::max<int64_t>(S, 1)), wide(seg->binary ? sizeof(uint32_t) * (size_t)S * seg->code_words : 0);
    if (S > 0 && seg->binary) {
        MQVS_HIP(hipMemcpyAsync(didx.p, idx32.data(), sizeof(int32_t) * S, hipMemcpyHostToDevice, s));
        launch_bivf_gather(seg->codes, seg->code_words, didx.as<int32_t>(), S, wide.as<uint32_t>(), s);
        MQVS_HIP(hipMemcpy2DAsync(buf.as<uint8_t>() + 32, (size_t)rb, wide.p, (size_t)seg->code_words * 4, (size_t)rb,
                                  (size_t)S, hipMemcpyDeviceToDevice, s));
    } else if (S > 0) {
        MQVS_HIP(hipMemcpyAsync(didx.p, idx64.data(), sizeof(int64_t) * S, hipMemcpyHostToDevice, s));
        launch_gather_rows(seg->rows, seg->d, seg->d, didx.as<int64_t>(), S, (float *)(buf.as<uint8_t>() + 32), s);
    }
    uint64_t *hash = out.as<uint64_t>();
    launch_block_checksum(buf.as<uint8_t>(), tab.as<IngestBlock>(), 1, 1, (int *)(hash + 2), hash, s);
    MQVS_HIP(hipGetLastError());
    uint64_t h[2] = {};
    MQVS_HIP(hipMemcpyAsync(h, hash, sizeof(h), hipMemcpyDeviceToHost, s));
    MQVS_HIP(hipStreamSynchronize(s));
    return h[0];
}

static int64_t blob_content_bytes(const mqvs_index *ix) {
    return (int64_t)sizeof(BlobHeader) + ix->nlist * row_bytes_of(ix->seg) + 4 * ix->seg->n;
}

size_t blob_bytes(const mqvs_index *ix) {
    const int64_t content = blob_content_bytes(ix);
    return (size_t)(content + kBlobFrame * ((content + kBlobBlock - 1) / kBlobBlock));
}

size_t save_impl(mqvs_index *ix, uint8_t *out, size_t cap) {
    if (!ix || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
    mqvs_segment *seg = ix->seg;
    const int64_t n = seg->n, L = ix->nlist, rb = row_bytes_of(seg), cb = L * rb;
    const int64_t content = blob_content_bytes(ix), nb = (content + kBlobBlock - 1) / kBlobBlock;
    const size_t total = blob_bytes(ix);
    if (cap < total)
        fail(MQVS_ERR_BAD_ARGUMENTS, "output holds " + std::to_string(cap) + " bytes, " + std::to_string(total) + " needed");
    DeviceGuard guard(seg->device);
    hipStream_t s = thread_stream(seg->device);
    BlobHeader hd{};
    std::memcpy(hd.magic, kBlobMagic, 8);
    hd.version = MQVS_INDEX_BLOB_VERSION;
    hd.kind = ix->binary ? MQVS_INDEX_KIND_BINARY_IVF : MQVS_INDEX_KIND_FLOAT_IVF;
    hd.metric = (uint32_t)ix->metric;
    hd.dim = (uint32_t)seg->d;
    hd.n = (uint64_t)n;
    hd.nlist = (uint64_t)L;
    std::memcpy(&hd.alpha_bits, &ix->alpha, 4);
    hd.np95 = (uint32_t)ix->np95;
    hd.fingerprint = segment_fingerprint(seg, s);
    hd.plane_fmt = ix->binary ? 0u : (uint32_t)ix->plane_fmt;

    // ---- the content: header, centroid table, canonical assignment
    TmpBuf cont((size_t)content), asg(sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1));
    uint8_t *c = cont.as<uint8_t>();
    MQVS_HIP(hipMemcpyAsync(c, &hd, sizeof(hd), hipMemcpyHostToDevice, s));
    if (ix->binary)
        MQVS_HIP(hipMemcpy2DAsync(c + sizeof(hd), (size_t)rb, ix->bcent, (size_t)seg->code_words * 4, (size_t)rb,
                                  (size_t)L, hipMemcpyDeviceToDevice, s));
    else
        MQVS_HIP(hipMemcpyAsync(c + sizeof(hd), ix->cent->rows, (size_t)cb, hipMemcpyDeviceToDevice, s));
    if (n > 0) {
        // the list of a position, scattered to its row; rows at no position: -1
        MQVS_HIP(hipMemsetAsync(asg.p, 0xFF, sizeof(int32_t) * (size_t)n, s));
        launch_grp_assign_of(ix->perm, ix->list_off, L, ix->npos, n, asg.as<int32_t>(), s);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(c + sizeof(hd) + cb, asg.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    // ---- the frame: method NONE blocks of at most kBlobBlock bytes
    TmpBuf framed(total), tab(sizeof(IngestBlock) * (size_t)nb), hashes(16 * (size_t)nb + 16);
    std::vector<uint8_t> heads((size_t)nb * kBlobFrame, 0);
    std::vector<IngestBlock> ht((size_t)nb);
    for (int64_t i = 0; i < nb; ++i) {
        const uint32_t len = (uint32_t)std::min(kBlobBlock, content - i * kBlobBlock);
        put_block_header(heads.data() + i * kBlobFrame + 16, len);
        ht[i].src = i * (kBlobBlock + kBlobFrame) + kBlobFrame;
        ht[i].dst = i * kBlobBlock;
        ht[i].csize = ht[i].usize = len;
        ht[i].method = 0x02;
        ht[i].pad = 0;
    }
    uint8_t *f = framed.as<uint8_t>();
    const size_t pitch = (size_t)(kBlobBlock + kBlobFrame);
    MQVS_HIP(hipMemcpy2DAsync(f, pitch, heads.data(), (size_t)kBlobFrame, (size_t)kBlobFrame, (size_t)nb,
                              hipMemcpyHostToDevice, s));
    const int64_t full = content / kBlobBlock, rest = content - full * kBlobBlock;
    if (full > 0)
        MQVS_HIP(hipMemcpy2DAsync(f + kBlobFrame, pitch, c, (size_t)kBlobBlock, (size_t)kBlobBlock, (size_t)full,
                                  hipMemcpyDeviceToDevice, s));
    if (rest > 0)
        MQVS_HIP(hipMemcpyAsync(f + full * pitch + kBlobFrame, c + full * kBlobBlock, (size_t)rest,
                                hipMemcpyDeviceToDevice, s));
    MQVS_HIP(hipMemcpyAsync(tab.p, ht.data(), sizeof(IngestBlock) * (size_t)nb, hipMemcpyHostToDevice, s));
    uint64_t *hash = hashes.as<uint64_t>();
    // (the verdict word of the checksum pass is not read: the stored checksums are still zero)
    launch_block_checksum(f, tab.as<IngestBlock>(), nb, 1, (int *)(hash + 2 * nb), hash, s);
    MQVS_HIP(hipGetLastError());
    MQVS_HIP(hipMemcpy2DAsync(f, pitch, hash, 16, 16, (size_t)nb, hipMemcpyDeviceToDevice, s));
    MQVS_HIP(hipMemcpyAsync(out, f, total, hipMemcpyDeviceToHost, s));
    MQVS_HIP(hipStreamSynchronize(s));
    return total;
}

// the header of a decoded blob; throws what the error table of include/mqvs.h names
static void check_blob_header(const BlobHeader &hd) {
    if (std::memcmp(hd.magic, kBlobMagic, 8) != 0) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: bad magic");
    if (hd.version != MQVS_INDEX_BLOB_VERSION)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "index blob: format version " + std::to_string(hd.version) + " is not implemented");
    float alpha;
    std::memcpy(&alpha, &hd.alpha_bits, 4);
    const bool fl = hd.kind == MQVS_INDEX_KIND_FLOAT_IVF, bi = hd.kind == MQVS_INDEX_KIND_BINARY_IVF;
    const bool metric_ok = fl ? (hd.metric == MQVS_METRIC_L2 || hd.metric == MQVS_METRIC_IP || hd.metric == MQVS_METRIC_COSINE)
                              : (hd.metric == MQVS_METRIC_HAMMING || hd.metric == MQVS_METRIC_JACCARD);
    if ((!fl && !bi) || !metric_ok || hd.nlist < 1 || hd.nlist > (1u << 20) || hd.n >= ((uint64_t)1 << 31) ||
        (hd.n > 0 && hd.nlist > hd.n) || !(alpha >= 1.0f && alpha <= 4.0f) || hd.np95 > (uint32_t)kSortCap ||
        hd.dim == 0 || hd.dim > (1u << 24) || (bi && hd.dim % 8) ||
        (hd.plane_fmt != MQVS_INDEX_PLANE_BF16 && (bi || hd.plane_fmt != MQVS_INDEX_PLANE_FP8)))
        fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: malformed header");
}

mqvs_index *load_impl(mqvs_segment *seg, const uint8_t *blob, size_t bytes) {
    if (!seg || !blob) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
    if (bytes < (size_t)kBlobFrame + sizeof(BlobHeader)) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: truncated");
    const int64_t n = seg->n, rb = row_bytes_of(seg);
    DeviceGuard guard(seg->device);
    hipStream_t s = thread_stream(seg->device);
    hipEvent_t e0, e1;
    MQVS_HIP(hipEventCreate(&e0));
    MQVS_HIP(hipEventCreate(&e1));
    mqvs_index *ix = nullptr;
    try {
        MQVS_HIP(hipEventRecord(e0, s));
        // ---- the block chain, its checksums, the decoded content
        const int64_t maxb = (int64_t)bytes / kBlobFrame + 1;
        TmpBuf dblob(bytes), tab(sizeof(IngestBlock) * (size_t)maxb), words(sizeof(int64_t) * 4);
        MQVS_HIP(hipMemcpyAsync(dblob.p, blob, bytes, hipMemcpyHostToDevice, s));
        launch_block_table(dblob.as<uint8_t>(), (int64_t)bytes, tab.as<IngestBlock>(), maxb, words.as<int64_t>(), s);
        MQVS_HIP(hipGetLastError());
        int64_t tb[3] = {};
        MQVS_HIP(hipMemcpyAsync(tb, words.p, sizeof(tb), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipStreamSynchronize(s));
        // (no codec expands more than 256-fold: a larger claim is not allocated)
        if (tb[2] || tb[1] < (int64_t)sizeof(BlobHeader) || tb[1] / 256 > (int64_t)bytes)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: truncated or malformed compressed block chain");
        const int64_t nblk = tb[0], total = tb[1];
        constexpr int kBadChecksum = 8;  // (the decode raises 4)
        int *status = (int *)(words.as<int64_t>() + 3);
        MQVS_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
        TmpBuf cont((size_t)total);
        uint8_t *c = cont.as<uint8_t>();
        launch_block_checksum(dblob.as<uint8_t>(), tab.as<IngestBlock>(), nblk, kBadChecksum, status, nullptr, s);
        launch_decode_blocks(dblob.as<uint8_t>(), (int64_t)bytes, tab.as<IngestBlock>(), nblk, c, status, s);
        MQVS_HIP(hipGetLastError());
        int hstatus = 0;
        BlobHeader hd{};
        MQVS_HIP(hipMemcpyAsync(&hstatus, status, sizeof(int), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipMemcpyAsync(&hd, c, sizeof(hd), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipStreamSynchronize(s));
        if (hstatus & kBadChecksum)
            fail(MQVS_ERR_CHECKSUM, "Checksum doesn't match: corrupted data (index blob, CityHash128 of a compressed block)");
        if (hstatus) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: malformed LZ4 block (CANNOT_DECOMPRESS)");
        // ---- the header against itself, then against the segment
        check_blob_header(hd);
        const bool binary = hd.kind == MQVS_INDEX_KIND_BINARY_IVF;
        const int64_t L = (int64_t)hd.nlist;
        const int64_t hrb = binary ? hd.dim / 8 : 4 * (int64_t)hd.dim, cb = L * hrb;
        if (total != (int64_t)sizeof(BlobHeader) + cb + 4 * (int64_t)hd.n)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: " + std::to_string(total) + " bytes of content, the header implies " +
                                              std::to_string((int64_t)sizeof(BlobHeader) + cb + 4 * (int64_t)hd.n));
        if (binary != seg->binary)
            fail(MQVS_ERR_LOGICAL, std::string("index blob: a ") + (binary ? "binary" : "Float32") + " index on a " +
                                       (seg->binary ? "binary" : "Float32") + " segment");
        if ((int64_t)hd.n != n || (int64_t)hd.dim != seg->d)
            fail(MQVS_ERR_LOGICAL, "index blob: saved over " + std::to_string(hd.n) + " rows of dimension " +
                                       std::to_string(hd.dim) + ", the segment has " + std::to_string(n) + " of " +
                                       std::to_string(seg->d));
        if (!binary && ((int)hd.metric == MQVS_METRIC_COSINE) != (seg->metric == MQVS_METRIC_COSINE))
            fail(MQVS_ERR_LOGICAL, "segment was prepared for a different metric (cosine segments are normalised in HBM)");
        if (!binary) check_index_width(seg);
        if (hd.fingerprint != segment_fingerprint(seg, s))
            fail(MQVS_ERR_LOGICAL, "index blob: saved over other rows than the segment's (fingerprint mismatch)");

        // ---- the index
        ix = new mqvs_index();
        ix->seg = seg;
        ix->binary = binary;
        ix->metric = (int)hd.metric;
        ix->nlist = L;
        std::memcpy(&ix->alpha, &hd.alpha_bits, 4);
        ix->np95 = (int)hd.np95;
        if (binary) {
            ix->coarse_metric = MQVS_METRIC_HAMMING;
            const size_t cwb = (size_t)seg->code_words * 4;
            ix->bcent = dalloc<uint32_t>(ix, (size_t)L * seg->code_words);
            MQVS_HIP(hipMemsetAsync(ix->bcent, 0, cwb * (size_t)L, s));
            MQVS_HIP(hipMemcpy2DAsync(ix->bcent, cwb, c + sizeof(hd), (size_t)rb, (size_t)rb, (size_t)L,
                                      hipMemcpyDeviceToDevice, s));
        } else {
            ix->coarse_metric = ix->metric == MQVS_METRIC_L2 ? MQVS_METRIC_L2 : kMetricIpRaw;
            ix->dpad = round_up(seg->d, kBfK);
            ix->plane_fmt = (int)hd.plane_fmt;
            ix->cent = segment_from_device((const float *)(c + sizeof(hd)), L, seg->d,
                                           ix->metric == MQVS_METRIC_L2 ? MQVS_METRIC_L2 : MQVS_METRIC_IP, s);
        }
        // (the assignment follows a binary centroid table at any byte offset)
        TmpBuf asg(sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1));
        if (n > 0)
            MQVS_HIP(hipMemcpyAsync(asg.p, c + sizeof(hd) + cb, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
        finish_index(ix, asg.as<int32_t>(), true, s);
        MQVS_HIP(hipEventRecord(e1, s));
        MQVS_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        MQVS_HIP(hipEventElapsedTime(&ms, e0, e1));
        ix->build_ms = ms;
        if (ix->cent) ix->bytes += ix->cent->bytes;
    } catch (...) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (ix) free_index(ix);
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ix;
}

// host only: the header of a blob whose first block is stored (method NONE)
void blob_info_impl(const uint8_t *blob, size_t bytes, mqvs_index_blob_info_t *out) {
    if (!blob || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
    if (bytes < (size_t)kBlobFrame + sizeof(BlobHeader)) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: truncated");
    const uint8_t *h = blob + 16;
    auto u32 = [](const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); };
    if (h[0] == 0x82) fail(MQVS_ERR_NOT_IMPLEMENTED, "index blob: the first block is LZ4-compressed (load it, or decompress it first)");
    const uint32_t csize = u32(h + 1), usize = u32(h + 5);
    if (h[0] != 0x02 || csize < 9 || csize - 9 != usize || usize < sizeof(BlobHeader) || 16 + (size_t)csize > bytes)
        fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: malformed first block");
    BlobHeader hd;
    std::memcpy(&hd, blob + kBlobFrame, sizeof(hd));
    check_blob_header(hd);
    std::memset(out, 0, sizeof(*out));
    out->version = hd.version;
    out->kind = hd.kind;
    out->metric = (int32_t)hd.metric;
    out->dim = (int32_t)hd.dim;
    out->n = (int64_t)hd.n;
    out->nlist = (int64_t)hd.nlist;
    std::memcpy(&out->alpha, &hd.alpha_bits, 4);
    out->np95 = (int32_t)hd.np95;
    out->fingerprint = hd.fingerprint;
    const int64_t hrb = hd.kind == MQVS_INDEX_KIND_BINARY_IVF ? hd.dim / 8 : 4 * (int64_t)hd.dim;
    out->content_bytes = (uint64_t)((int64_t)sizeof(BlobHeader) + (int64_t)hd.nlist * hrb + 4 * (int64_t)hd.n);
}

}  // namespace mqvs
