// JPEG decode, the data-parallel half: quantised coefficients (csrc/jpeg_entropy.h decodes them on loader threads) ->
// uint8 HWC pixels in the staging buffer that bsclip_augment_images reads.  One launch sequence serves a batch of images of mixed
// sizes and sampling modes; blockIdx.y is the image, its 16-int record (jpeg_entropy.h, Frame::write_record) says where its
// coefficients and pixels live.
//
// All arithmetic is integer and is libjpeg's default decoder, rounding biases included, so that tests/jpeg_model.py (NumPy) agrees
// bit for bit and PIL agrees on every fixture:
//   pass 1  dequantise (coef x table) + the slow-integer LL&M inverse DCT (jidctint.c: 13-bit constants, columns first with 2 extra
//           bits kept, rows second, descale by 13 + 2 + 3 bits, + 128, clamp through libjpeg's 10-bit range mask) -> planar uint8
//           Y / Cb / Cr in scratch, each plane padded to whole MCUs;
//   pass 2  "fancy" triangle upsampling of the chroma planes (jdsample.c: 3/4 : 1/4 per axis, biases 8 / 7 for h2v2, 1 / 2 for h2v1
//           and h1v2, neighbours clamped at the component's real downsampled size ceil(W / h) x ceil(H / v); plain replication when a
//           horizontally subsampled component is no more than 2 samples wide, as libjpeg does) + BT.601 full-range YCbCr -> RGB in
//           16-bit fixed point (jdcolor.c) -> HWC bytes.  Grey replicates Y.
// Neither kernel has a loop or an address that depends on image DATA: everything is derived from the record, which
// bsclip_jpeg_pixels validates on the host (records_host) and then copies to the device itself, so what the kernels read is what
// was checked.
#include "common.h"
#include "jpeg_entropy.h"

namespace {

constexpr int REC = bsclip_jpeg::REC;
constexpr int BLOCKS_PER_WG = 32;   // 8 threads per 8x8 block, 256 threads
constexpr int WS_LD = 72;           // int32 per block in LDS: 64 + 8 pad.  The column pass (ds_read2_b32 / ds_write2_b32, banks modulo 32 per
                                    // 32-lane half = 4 blocks x 8 columns) then touches 32 distinct banks: conflict-free.  The dequantise
                                    // store and the row read are 2 + 2 ds_write_b128 / ds_read_b128 of a lane's own 8 dwords; their 16-byte
                                    // slots are 18 b + 2 k (block b, row k) modulo 16 per 256-byte bank row, so rows of neighbouring blocks
                                    // in a 16-lane group can alias two ways.  Not measured; a 68-dword stride would clear those four
                                    // instructions and make the sixteen of the column pass 2-way instead.

struct Geom {
    long coef_off, out_off;
    int W, H, ncomp, hs, vs, mcus_x, mcus_y;
    int n0, nc;    // blocks of the luma plane, of each chroma plane
};
__device__ __forceinline__ Geom load_geom(const int* r) {
    Geom g;
    g.coef_off = (long)(unsigned)r[0] | ((long)r[1] << 32);
    g.out_off = (long)(unsigned)r[2] | ((long)r[3] << 32);
    g.W = r[4], g.H = r[5], g.ncomp = r[6], g.hs = r[7], g.vs = r[8];
    g.mcus_x = (g.W + 8 * g.hs - 1) / (8 * g.hs);
    g.mcus_y = (g.H + 8 * g.vs - 1) / (8 * g.vs);
    g.nc = g.mcus_x * g.mcus_y;
    g.n0 = g.nc * g.hs * g.vs;
    return g;
}

// jidctint.c, CONST_BITS = 13
constexpr unsigned F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
                   F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// one 8-point pass of jpeg_idct_islow; out[i] = (.. + (1 << (SHIFT - 1))) >> SHIFT.  The sums and products are formed modulo 2^32
// (unsigned) and read as two's complement for the arithmetic shift: identical to libjpeg for every stream whose values fit 32 bits
// -- all that an 8-bit image can encode -- and DEFINED, wrapping, for the rest (16-bit table entries times full-range
// coefficients); tests/jpeg_model.py wraps its int32 the same way, so kernel and model agree on those too.
template <int SHIFT>
__device__ __forceinline__ void idct8(const int v[8], int out[8]) {
    unsigned in[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) in[j] = (unsigned)v[j];
    unsigned z1 = (in[2] + in[6]) * F_0_541;
    const unsigned t2 = z1 - in[6] * F_1_847, t3 = z1 + in[2] * F_0_765;
    const unsigned t0 = (in[0] + in[4]) << 13, t1 = (in[0] - in[4]) << 13;   // << CONST_BITS
    const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    unsigned o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
    z1 = o0 + o3;
    unsigned z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const unsigned z5 = (z3 + z4) * F_1_175;
    o0 *= F_0_298, o1 *= F_2_053, o2 *= F_3_072, o3 *= F_1_501;
    z1 *= 0u - F_0_899, z2 *= 0u - F_2_562, z3 *= 0u - F_1_961, z4 *= 0u - F_0_390;
    z3 += z5, z4 += z5;
    o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
    constexpr unsigned R = 1u << (SHIFT - 1);
    auto descale = [](unsigned x) { return (int)(x + R) >> SHIFT; };
    out[0] = descale(t10 + o3), out[7] = descale(t10 - o3);
    out[1] = descale(t11 + o2), out[6] = descale(t11 - o2);
    out[2] = descale(t12 + o1), out[5] = descale(t12 - o1);
    out[3] = descale(t13 + o0), out[4] = descale(t13 - o0);
}
// libjpeg's IDCT range limit: sample_range_limit[128 + (v & 1023)] -- clamp(v + 128, 0, 255) for every v a valid stream produces
__device__ __forceinline__ unsigned range_limit(int v) {
    const int x = v & 1023;
    return (unsigned)(x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896);
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef, const unsigned short* __restrict__ qtab,
                                                        const int* __restrict__ rec, unsigned char* __restrict__ scratch) {
    __shared__ int ws[BLOCKS_PER_WG * WS_LD];
    const int* r = rec + blockIdx.y * REC;
    const Geom g = load_geom(r);
    const int nblocks = g.n0 + (g.ncomp == 3 ? 2 * g.nc : 0);
    if ((int)blockIdx.x * BLOCKS_PER_WG >= nblocks) return;   // uniform over the workgroup: images smaller than the batch's largest
    const int lb = threadIdx.x >> 3, k = threadIdx.x & 7;
    const int blk = blockIdx.x * BLOCKS_PER_WG + lb;
    const bool live = blk < nblocks;
    int* w = ws + lb * WS_LD;
    if (live) {
        const int c = blk < g.n0 ? 0 : (blk < g.n0 + g.nc ? 1 : 2);
        const u16x8 cv = *reinterpret_cast<const u16x8*>(coef + g.coef_off + (long)blk * 64 + k * 8);
        const u16x8 qv = *reinterpret_cast<const u16x8*>(qtab + (long)r[9 + c] * 64 + k * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) w[k * 8 + j] = (int)(short)cv[j] * (int)qv[j];   // |.| <= 2^15 x (2^16 - 1): fits
    }
    BSCLIP_LDS_BARRIER();
    if (live) {   // column k of the block, in place: no other thread touches this column
        int in[8], out[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) in[j] = w[j * 8 + k];
        idct8<13 - 2>(in, out);
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j * 8 + k] = out[j];
    }
    BSCLIP_LDS_BARRIER();
    if (live) {   // row k -> 8 bytes of the component's plane
        int in[8], out[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) in[j] = w[k * 8 + j];
        idct8<13 + 2 + 3>(in, out);
        const int c = blk < g.n0 ? 0 : (blk < g.n0 + g.nc ? 1 : 2);
        const int local = c == 0 ? blk : blk - g.n0 - (c - 1) * g.nc;
        const int bw = c == 0 ? g.mcus_x * g.hs : g.mcus_x;
        const int by = local / bw, bx = local - by * bw;
        const long plane = g.coef_off + (c == 0 ? 0 : (long)(g.n0 + (c - 1) * g.nc) * 64);
        uint2 v;
        v.x = range_limit(out[0]) | (range_limit(out[1]) << 8) | (range_limit(out[2]) << 16) | (range_limit(out[3]) << 24);
        v.y = range_limit(out[4]) | (range_limit(out[5]) << 8) | (range_limit(out[6]) << 16) | (range_limit(out[7]) << 24);
        *reinterpret_cast<uint2*>(scratch + plane + ((long)(by * 8 + k) * bw + bx) * 8) = v;
    }
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one chroma sample at full resolution.  mode: 0 copy / replicate, 1 fancy h2v1, 2 fancy h1v2, 3 fancy h2v2
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ pl, int pw, int x, int y, int hs, int vs, int dw, int dh,
                                         int mode) {
    const int cx = hs == 2 ? x >> 1 : x, cy = vs == 2 ? y >> 1 : y;
    const int a = pl[(long)cy * pw + cx];
    if (mode == 0) return a;
    const int nx = (x & 1) ? min(cx + 1, dw - 1) : max(cx - 1, 0);
    const int ny = (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);
    if (mode == 1) return (3 * a + pl[(long)cy * pw + nx] + ((x & 1) ? 2 : 1)) >> 2;
    if (mode == 2) return (3 * a + pl[(long)ny * pw + cx] + ((y & 1) ? 2 : 1)) >> 2;
    const int here = 3 * a + pl[(long)ny * pw + cx], next = 3 * pl[(long)cy * pw + nx] + pl[(long)ny * pw + nx];
    return (3 * here + next + ((x & 1) ? 7 : 8)) >> 4;
}

// 256 consecutive pixels of one image per workgroup (an HWC image is one flat run of W*H pixels).  The 768 bytes are assembled in
// LDS at the byte phase of their global address and leave as aligned dwords; only the first and last dword of a run, which it may
// share with its neighbours, go out bytewise.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const unsigned char* __restrict__ scratch, const int* __restrict__ rec,
                                                         unsigned char* __restrict__ out) {
    __shared__ unsigned stage[(768 + 4) / 4];
    const Geom g = load_geom(rec + blockIdx.y * REC);
    const long npix = (long)g.W * g.H;
    const long p0 = (long)blockIdx.x * 256;
    if (p0 >= npix) return;   // uniform over the workgroup
    const int count = (int)min((long)256, npix - p0);
    const long a = g.out_off + 3 * p0;   // first byte of the run, relative to `out` (16-byte aligned)
    const int lead = (int)(a & 3);
    unsigned char* sb = reinterpret_cast<unsigned char*>(stage);
    const int t = threadIdx.x;
    if (t < count) {
        const long p = p0 + t;
        const int y = (int)(p / g.W), x = (int)(p - (long)y * g.W);
        const unsigned char* base = scratch + g.coef_off;
        const int pw0 = g.mcus_x * g.hs * 8;
        const int Y = base[(long)y * pw0 + x];
        int R = Y, G = Y, B = Y;
        if (g.ncomp == 3) {
            const int dw = (g.W + g.hs - 1) / g.hs, dh = (g.H + g.vs - 1) / g.vs;
            const bool fancy_h = g.hs == 2 && dw > 2;
            const int mode = g.hs == 2 ? (fancy_h ? (g.vs == 2 ? 3 : 1) : 0) : (g.vs == 2 ? 2 : 0);
            const int pwc = g.mcus_x * 8;
            const unsigned char* cbp = base + (long)g.n0 * 64;
            const unsigned char* crp = cbp + (long)g.nc * 64;
            const int cb = chroma_at(cbp, pwc, x, y, g.hs, g.vs, dw, dh, mode) - 128;
            const int cr = chroma_at(crp, pwc, x, y, g.hs, g.vs, dw, dh, mode) - 128;
            // jdcolor.c build_ycc_rgb_table: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554
            R = clamp255(Y + ((91881 * cr + 32768) >> 16));
            G = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
            B = clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
        sb[lead + 3 * t + 0] = (unsigned char)R;
        sb[lead + 3 * t + 1] = (unsigned char)G;
        sb[lead + 3 * t + 2] = (unsigned char)B;
    }
    BSCLIP_LDS_BARRIER();
    const int span = lead + 3 * count;   // LDS byte i is global byte (a - lead) + i; [lead, span) is this run's
    if (4 * t < span) {
        unsigned char* dst = out + (a - lead) + 4 * t;
        if (4 * t >= lead && 4 * t + 4 <= span) {
            *reinterpret_cast<unsigned*>(dst) = stage[t];
        } else {
            for (int j = 0; j < 4; ++j)
                if (4 * t + j >= lead && 4 * t + j < span) dst[j] = sb[4 * t + j];
        }
    }
}

int set_jpeg_error(int rc, const char* who, const char* msg) {
    bsclip_set_error("%s: %s", who, msg);
    return rc;
}

}  // namespace

extern "C" int bsclip_jpeg_probe(const void* bytes, int64_t n, bsclip_jpeg_info* info_out) {
    BSCLIP_REQUIRE(bytes && info_out && n > 0, "bsclip_jpeg_probe: null/empty input");
    bsclip_jpeg::Decoder d;
    const int rc = d.parse(static_cast<const uint8_t*>(bytes), (size_t)n);
    if (rc) return set_jpeg_error(rc, "bsclip_jpeg_probe", d.msg);
    const bsclip_jpeg::Frame& f = d.f;
    *info_out = bsclip_jpeg_info{f.width, f.height, f.ncomp, f.hs, f.vs, f.restart, f.coef_count, f.pixel_bytes};
    return BSCLIP_OK;
}

extern "C" int bsclip_jpeg_entropy_decode(const void* bytes, int64_t n, int16_t* coef_out, int64_t coef_capacity, uint16_t* qtab_out,
                                          int32_t* record_out) {
    BSCLIP_REQUIRE(bytes && coef_out && qtab_out && record_out && n > 0 && coef_capacity > 0,
                   "bsclip_jpeg_entropy_decode: null/empty input");
    char msg[160];
    const int rc = bsclip_jpeg::entropy_decode(static_cast<const uint8_t*>(bytes), (size_t)n, coef_out, coef_capacity, qtab_out,
                                               record_out, msg, sizeof(msg));
    if (rc) return set_jpeg_error(rc, "bsclip_jpeg_entropy_decode", msg);
    return BSCLIP_OK;
}

extern "C" int64_t bsclip_jpeg_pixels_workspace_bytes(int64_t coef_count) { return coef_count > 0 ? coef_count : -1; }

extern "C" int bsclip_jpeg_pixels(const int16_t* coef_dev, int64_t coef_count, const uint16_t* qtab_dev, int qtab_slots,
                                  const int32_t* records_host, int32_t* records_dev, int B, void* scratch, int64_t scratch_bytes,
                                  void* out_u8, int64_t out_capacity, void* stream) {
    BSCLIP_REQUIRE(coef_dev && qtab_dev && records_host && records_dev && scratch && out_u8, "bsclip_jpeg_pixels: null pointer");
    BSCLIP_REQUIRE(B >= 1 && B <= 65535 && coef_count > 0 && qtab_slots > 0 && out_capacity > 0,
                   "bsclip_jpeg_pixels: B=%d coef_count=%lld qtab_slots=%d out_capacity=%lld", B, (long long)coef_count, qtab_slots,
                   (long long)out_capacity);
    BSCLIP_REQUIRE(aligned_to(16, coef_dev, qtab_dev) && aligned_to(16, scratch, out_u8) && aligned_to(4, records_dev),
                   "bsclip_jpeg_pixels: coef, qtab, scratch and out must be 16-byte aligned, records 4-byte aligned");
    BSCLIP_REQUIRE(scratch_bytes >= coef_count, "bsclip_jpeg_pixels: scratch_bytes=%lld < bsclip_jpeg_pixels_workspace_bytes = %lld",
                   (long long)scratch_bytes, (long long)coef_count);
    int64_t max_blocks = 0, max_pixels = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* r = records_host + (size_t)b * REC;
        const int64_t coef_off = (int64_t)(uint32_t)r[0] | ((int64_t)r[1] << 32), out_off = (int64_t)(uint32_t)r[2] | ((int64_t)r[3] << 32);
        const int64_t blocks = bsclip_jpeg::record_blocks(r[4], r[5], r[6], r[7], r[8]);
        BSCLIP_REQUIRE(blocks > 0, "bsclip_jpeg_pixels: record %d: W=%d H=%d components=%d sampling=%dx%d is not decodable", b, r[4], r[5],
                       r[6], r[7], r[8]);
        BSCLIP_REQUIRE(blocks == r[12], "bsclip_jpeg_pixels: record %d: %d blocks recorded but its sizes imply %lld", b, r[12],
                       (long long)blocks);
        BSCLIP_REQUIRE(coef_off >= 0 && coef_off % 64 == 0 && coef_off <= coef_count - blocks * 64,
                       "bsclip_jpeg_pixels: record %d: coefficients [%lld, +%lld) outside coef_count=%lld (or not a multiple of 64)", b,
                       (long long)coef_off, (long long)blocks * 64, (long long)coef_count);
        const int64_t pix = (int64_t)r[4] * r[5];
        BSCLIP_REQUIRE(out_off >= 0 && out_off <= out_capacity - 3 * pix,
                       "bsclip_jpeg_pixels: record %d: pixels [%lld, +%lld) outside out_capacity=%lld", b, (long long)out_off,
                       (long long)(3 * pix), (long long)out_capacity);
        for (int c = 0; c < r[6]; ++c)
            BSCLIP_REQUIRE(r[9 + c] >= 0 && r[9 + c] < qtab_slots, "bsclip_jpeg_pixels: record %d: table slot %d outside qtab_slots=%d", b,
                           r[9 + c], qtab_slots);
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        max_pixels = pix > max_pixels ? pix : max_pixels;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the kernels read exactly the records that were just validated: the library makes the device copy itself, in stream order
    const hipError_t ce = hipMemcpyAsync(records_dev, records_host, (size_t)B * REC * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (ce != hipSuccess) {
        bsclip_set_error("bsclip_jpeg_pixels: copying the records failed: %s", hipGetErrorString(ce));
        return BSCLIP_ERR_LAUNCH;
    }
    const dim3 g1((unsigned)((max_blocks + BLOCKS_PER_WG - 1) / BLOCKS_PER_WG), B);
    hipLaunchKernelGGL(jpeg_idct_kernel, g1, dim3(256), 0, s, reinterpret_cast<const short*>(coef_dev), qtab_dev, records_dev,
                       static_cast<unsigned char*>(scratch));
    const dim3 g2((unsigned)((max_pixels + 255) / 256), B);
    hipLaunchKernelGGL(jpeg_color_kernel, g2, dim3(256), 0, s, static_cast<const unsigned char*>(scratch), records_dev,
                       static_cast<unsigned char*>(out_u8));
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
