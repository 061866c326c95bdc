// JPEG decode, the entropy half on the device: a batch's streams as they are stored + each image's sync index -> the
// coefficient raster that bsclip_jpeg_entropy_decode writes on the host, which bsclip_jpeg_pixels then reads unchanged.
//
// blockIdx.y is the image, the x dimension covers its segments, one lane decodes one segment with the routine of jpeg_segment.h
// (shared with the host, where it runs under sanitisers).  A workgroup is one wave: a 256 x 341 image at sync_mcus = 4 has 88
// segments, so wider groups would mostly idle, and the four Huffman tables of the image (5 680 bytes) sit in its LDS.
//
// Zeros: each lane zero-fills a block (eight 16-byte stores to its own 128 bytes) immediately before it decodes that block's few
// non-zero coefficients into it, instead of a memset launch over the batch or staging blocks through LDS.  The segment's MCUs
// follow from the record, not from the data or from the index, and after a fault a lane keeps zero-filling to the end of its
// segment, so every element of every image's range is defined after the launch whatever the bytes hold.  LDS staging would need
// 128 bytes per lane for stores that are already whole, aligned 128-byte lines per lane.
//
// Nothing here trusts device data for an address: byte, index, table and coefficient ranges come from the records, which
// bsclip_jpeg_entropy_device validates on the host and then copies to the device itself; the reader is bounded by the image's byte
// range, table look-ups by the table's size, writes by the segment's blocks.
#include "common.h"
#include "jpeg_entropy.h"

namespace {

using namespace bsclip_jpeg;
constexpr int EREC = 8;   // int32 per image: byte offset, byte length, first index entry, entries, sync_mcus, table slot, 0, 0
constexpr int LANES = 64;

__global__ __launch_bounds__(LANES) void jpeg_entropy_kernel(const uint8_t* __restrict__ bytes, const int32_t* __restrict__ sync,
                                                              const uint32_t* __restrict__ huff, const int* __restrict__ rec,
                                                              const int* __restrict__ erec, int16_t* __restrict__ coef,
                                                              int* __restrict__ status) {
    __shared__ SegHuff tabs[SEG_TABLES];
    const int* r = rec + blockIdx.y * REC;
    const int* e = erec + blockIdx.y * EREC;
    const int nent = e[3];
    if ((int)blockIdx.x * LANES >= nent) return;   // uniform over the workgroup: images with fewer segments than the batch's largest
    constexpr int TAB_DWORDS = SEG_TABLES * (int)sizeof(SegHuff) / 4;
    const uint32_t* src = huff + (long)e[5] * TAB_DWORDS;
    uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
    for (int i = threadIdx.x; i < TAB_DWORDS; i += LANES) dst[i] = src[i];
    BSCLIP_LDS_BARRIER();
    const int seg = blockIdx.x * LANES + threadIdx.x;
    if (seg >= nent) return;
    SegGeom g;
    g.ncomp = r[6], g.hs = r[7], g.vs = r[8];
    g.mcus_x = (r[4] + 8 * g.hs - 1) / (8 * g.hs);
    g.nmcu = g.mcus_x * ((r[5] + 8 * g.vs - 1) / (8 * g.vs));
    g.sel = r[14];
    int first, count;
    bool chained;
    segment_range(seg, g.nmcu, r[13], e[4], &first, &count, &chained);
    const int4 ent = *reinterpret_cast<const int4*>(sync + ((long)e[2] + seg) * SYNC_ENTRY);
    int4 nxt = ent;
    if (chained) nxt = *reinterpret_cast<const int4*>(sync + ((long)e[2] + seg + 1) * SYNC_ENTRY);
    const int32_t entry[SYNC_ENTRY] = {ent.x, ent.y, ent.z, ent.w}, next[SYNC_ENTRY] = {nxt.x, nxt.y, nxt.z, nxt.w};
    const long coef_off = (long)(unsigned)r[0] | ((long)r[1] << 32);
    const int st = decode_segment_checked<true>(bytes + (unsigned)e[0], (uint32_t)e[1], entry, first, count, g, tabs, coef + coef_off,
                                                next, chained);
    if (st) atomicOr(status + blockIdx.y, st);
}

}  // namespace

extern "C" int64_t bsclip_jpeg_sync_index(const void* bytes, int64_t n, int sync_mcus, int32_t* index_out, int64_t capacity) {
    BSCLIP_REQUIRE(bytes && n > 0 && (index_out == nullptr || capacity > 0), "bsclip_jpeg_sync_index: null/empty input");
    char msg[160];
    const int64_t rc = sync_index(static_cast<const uint8_t*>(bytes), (size_t)n, sync_mcus, index_out, capacity, msg, sizeof(msg));
    if (rc < 0) bsclip_set_error("bsclip_jpeg_sync_index: %s", msg);
    return rc;
}

extern "C" int bsclip_jpeg_device_tables(const void* bytes, int64_t n, void* huff_out, uint16_t* qtab_out, int32_t* record_out) {
    BSCLIP_REQUIRE(bytes && huff_out && qtab_out && record_out && n > 0, "bsclip_jpeg_device_tables: null/empty input");
    BSCLIP_REQUIRE(aligned_to(4, huff_out), "bsclip_jpeg_device_tables: huff_out must be 4-byte aligned");
    char msg[160];
    const int rc = device_tables(static_cast<const uint8_t*>(bytes), (size_t)n, static_cast<SegHuff*>(huff_out), qtab_out, record_out, msg,
                                 sizeof(msg));
    if (rc) bsclip_set_error("bsclip_jpeg_device_tables: %s", msg);
    return rc;
}

extern "C" int bsclip_jpeg_entropy_device(const void* bytes_dev, int64_t bytes_capacity, const int32_t* sync_dev, int64_t sync_entries,
                                          const void* huff_dev, int huff_slots, const int32_t* records_host,
                                          const int32_t* segments_host, int32_t* records_dev, int32_t* segments_dev, int B,
                                          int16_t* coef_dev, int64_t coef_count, int32_t* status_dev, void* stream) {
    BSCLIP_REQUIRE(bytes_dev && sync_dev && huff_dev && records_host && segments_host && records_dev && segments_dev && coef_dev && status_dev,
                   "bsclip_jpeg_entropy_device: null pointer");
    BSCLIP_REQUIRE(B >= 1 && B <= 65535 && bytes_capacity > 0 && bytes_capacity <= 0x7fffffff && sync_entries > 0 && huff_slots > 0 &&
                       coef_count > 0,
                   "bsclip_jpeg_entropy_device: B=%d bytes_capacity=%lld sync_entries=%lld huff_slots=%d coef_count=%lld", B,
                   (long long)bytes_capacity, (long long)sync_entries, huff_slots, (long long)coef_count);
    BSCLIP_REQUIRE(aligned_to(16, sync_dev, coef_dev) && aligned_to(4, huff_dev) && aligned_to(4, records_dev, segments_dev, status_dev),
                   "bsclip_jpeg_entropy_device: sync and coef must be 16-byte aligned, huff, records, segments and status 4-byte aligned");
    int64_t max_entries = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* r = records_host + (size_t)b * REC;
        const int32_t* e = segments_host + (size_t)b * EREC;
        const int64_t coef_off = (int64_t)(uint32_t)r[0] | ((int64_t)r[1] << 32);
        const int64_t blocks = record_blocks(r[4], r[5], r[6], r[7], r[8]);
        BSCLIP_REQUIRE(blocks > 0, "bsclip_jpeg_entropy_device: record %d: W=%d H=%d components=%d sampling=%dx%d is not decodable", b, r[4],
                       r[5], r[6], r[7], r[8]);
        BSCLIP_REQUIRE(blocks == r[12], "bsclip_jpeg_entropy_device: record %d: %d blocks recorded but its sizes imply %lld", b, r[12],
                       (long long)blocks);
        BSCLIP_REQUIRE(coef_off >= 0 && coef_off % 64 == 0 && coef_off <= coef_count - blocks * 64,
                       "bsclip_jpeg_entropy_device: record %d: coefficients [%lld, +%lld) outside coef_count=%lld (or not a multiple of 64)", b,
                       (long long)coef_off, (long long)blocks * 64, (long long)coef_count);
        BSCLIP_REQUIRE(r[13] >= 0 && r[13] <= 65535 && (r[14] & ~0x77) == 0,
                       "bsclip_jpeg_entropy_device: record %d: restart interval %d / table selector word 0x%x out of range", b, r[13], r[14]);
        BSCLIP_REQUIRE(e[0] >= 0 && e[1] >= 1 && e[1] < MAX_STREAM && (int64_t)e[0] + e[1] <= bytes_capacity,
                       "bsclip_jpeg_entropy_device: record %d: bytes [%d, +%d) outside bytes_capacity=%lld (or 2^28 bytes and more)", b, e[0],
                       e[1], (long long)bytes_capacity);
        BSCLIP_REQUIRE(e[4] >= 1, "bsclip_jpeg_entropy_device: record %d: sync_mcus=%d must be at least 1", b, e[4]);
        const int nmcu = (int)(blocks / (r[7] * r[8] + (r[6] == 3 ? 2 : 0)));
        const int want = segment_count(nmcu, r[13], e[4]);
        BSCLIP_REQUIRE(e[3] == want, "bsclip_jpeg_entropy_device: record %d: %d index entries but %d MCUs, restart interval %d and sync_mcus=%d imply %d",
                       b, e[3], nmcu, r[13], e[4], want);
        BSCLIP_REQUIRE(e[2] >= 0 && (int64_t)e[2] + e[3] <= sync_entries,
                       "bsclip_jpeg_entropy_device: record %d: index entries [%d, +%d) outside sync_entries=%lld", b, e[2], e[3],
                       (long long)sync_entries);
        BSCLIP_REQUIRE(e[5] >= 0 && e[5] < huff_slots, "bsclip_jpeg_entropy_device: record %d: table slot %d outside huff_slots=%d", b, e[5],
                       huff_slots);
        max_entries = e[3] > max_entries ? e[3] : max_entries;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the kernel reads exactly the records that were just validated: the library makes the device copies itself, in stream order
    hipError_t ce = hipMemcpyAsync(records_dev, records_host, (size_t)B * REC * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (ce == hipSuccess) ce = hipMemcpyAsync(segments_dev, segments_host, (size_t)B * EREC * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (ce == hipSuccess) ce = hipMemsetAsync(status_dev, 0, (size_t)B * sizeof(int32_t), s);
    if (ce != hipSuccess) {
        bsclip_set_error("bsclip_jpeg_entropy_device: copying the records failed: %s", hipGetErrorString(ce));
        return BSCLIP_ERR_LAUNCH;
    }
    const dim3 grid((unsigned)((max_entries + LANES - 1) / LANES), B);
    hipLaunchKernelGGL(jpeg_entropy_kernel, grid, dim3(LANES), 0, s, static_cast<const uint8_t*>(bytes_dev), sync_dev,
                       static_cast<const uint32_t*>(huff_dev), records_dev, segments_dev, coef_dev, status_dev);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
