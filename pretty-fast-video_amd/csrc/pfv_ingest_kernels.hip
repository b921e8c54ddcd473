// pfv_ingest_kernels.hip -- the first step of an encoder: n_streams interleaved RGB8 / RGBA8 / BGRA8 pictures with a row pitch as packed
// planar Y | U | V 4:2:0 frames (k_ingest_rgb), the mirror of k_present_rgb.  Arithmetic: include/pfv_hip_ext.h, "RGB / RGBA picture input"
// (normative) -- the reference's load_frame (src/lib.rs:337-359) + VideoFrame::from_planes, the expressions of k_rgb_to_yuv420 -- and the
// chroma modes: POINT (the chroma of the even pixel, as the reference) or BOX (the mean of the 2 x 2 pixels' u8 chroma).  A streaming kernel:
// every source byte is read once, every destination byte written once, no atomics, no LDS.
// Included by pfv_capi.hip behind pfv_present_kernels.hip (kPix*, present_put); the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

constexpr int kChromaPoint = 0, kChromaBox = 1;   // PFV_CHROMA_* (include/pfv_hip_ext.h)

struct IngestSrc {
    const uint8_t *base;
    long pitch;      // bytes between the rows of a picture
    long stride;     // bytes between the pictures of consecutive streams
};

// JPEG-conversion RGB -> YCbCr in f32, left to right, no contraction; the caller converts as Rust's `as u8`
__device__ __forceinline__ float ingest_y(float r, float g, float b)
{
#pragma clang fp contract(off)
    return ((0.299f * r) + (0.587f * g)) + (0.114f * b);
}
__device__ __forceinline__ float ingest_u(float r, float g, float b)
{
#pragma clang fp contract(off)
    return ((128.0f - (0.168736f * r)) - (0.331264f * g)) + (0.5f * b);
}
__device__ __forceinline__ float ingest_v(float r, float g, float b)
{
#pragma clang fp contract(off)
    return ((128.0f + (0.5f * r)) - (0.418688f * g)) - (0.081312f * b);
}

// The byte-granular path: the 2 x 2 pixels of one chroma sample, byte loads and byte stores.
template <int FMT, int CHROMA>
__device__ __forceinline__ void ingest_quad_bytes(const uint8_t *pic, long pitch, int x, int y, uint8_t *py, uint8_t *pu, uint8_t *pv, int w)
{
    constexpr int bpp = FMT == kPixRgb8 ? 3 : 4;
    unsigned su = 0, sv = 0;
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const uint8_t *p = pic + (long)(y + dy) * pitch + (long)(x + dx) * bpp;
            const float r = (float)p[FMT == kPixBgra8 ? 2 : 0], g = (float)p[1], b = (float)p[FMT == kPixBgra8 ? 0 : 2];
            py[(long)(y + dy) * w + x + dx] = (uint8_t)f32_as_u8(ingest_y(r, g, b));
            if (CHROMA == kChromaBox || (dy == 0 && dx == 0)) {
                su += f32_as_u8(ingest_u(r, g, b));
                sv += f32_as_u8(ingest_v(r, g, b));
            }
        }
    const long c = (long)(y >> 1) * (w >> 1) + (x >> 1);
    pu[c] = (uint8_t)(CHROMA == kChromaBox ? (su + 2) >> 2 : su);
    pv[c] = (uint8_t)(CHROMA == kChromaBox ? (sv + 2) >> 2 : sv);
}

__device__ __forceinline__ uint2 ld_stream(const uint2 *p) { return make_uint2(__builtin_nontemporal_load(&p->x), __builtin_nontemporal_load(&p->y)); }
__device__ __forceinline__ void st_stream(uint2 *p, const uint2 &v)
{
    __builtin_nontemporal_store(v.x, &p->x); __builtin_nontemporal_store(v.y, &p->y);
}

// the 8 pixels of one row of a group: 24 bytes as three 8-byte loads (RGB8), 32 bytes as two 16-byte loads (the 4-byte formats)
template <int FMT>
__device__ __forceinline__ void ingest_load8(const uint8_t *p, unsigned (&w)[8])
{
    if (FMT == kPixRgb8) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint2 t = ld_stream(reinterpret_cast<const uint2 *>(p) + k);
            w[2 * k] = t.x; w[2 * k + 1] = t.y;
        }
        w[6] = w[7] = 0;
    } else {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint4 t = ld_stream(reinterpret_cast<const uint4 *>(p) + k);
            w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w;
        }
    }
}
// byte i of the loaded row as f32 (i is a constant after unrolling: one v_cvt_f32_ubyteN)
__device__ __forceinline__ float ingest_byte(const unsigned (&w)[8], int i) { return (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu); }
// pixel k of the loaded row; the alpha byte of the 4-byte formats is not looked at
template <int FMT>
__device__ __forceinline__ void ingest_px(const unsigned (&w)[8], int k, float &r, float &g, float &b)
{
    constexpr int bpp = FMT == kPixRgb8 ? 3 : 4;
    r = ingest_byte(w, bpp * k + (FMT == kPixBgra8 ? 2 : 0));
    g = ingest_byte(w, bpp * k + 1);
    b = ingest_byte(w, bpp * k + (FMT == kPixBgra8 ? 0 : 2));
}

constexpr int kIngestPairs = 2;   // row pairs per thread

// One thread owns a column of kIngestPairs groups of 8 x 2 pixels (the index division is paid once for 32 pixels); a group is two picture rows
// of 8 pixels, its two luma rows of 8 bytes and the four chroma samples under them.  Columns are numbered in raster order inside a picture
// (groups_x per band of kIngestPairs row pairs); blockIdx.y is the stream.
//   wide (decided per launch on the host, pfv_ingest.hip): the width is a multiple of 8 and picture rows and frames are aligned for it.  A
//   lane then loads each row of its group as 24 bytes (three 8-byte loads) or 32 bytes (two 16-byte loads), all non-temporal, the lanes of a
//   wavefront reading one contiguous span of 1536 or 2048 bytes per row, and stores each luma row as one 8-byte and U and V as one 4-byte
//   non-temporal store each.  Bytes are made with present_put (v_trunc_f32 + v_cvt_pk_u8_f32: exact for `as u8`, pfv_present_kernels.hip);
//   BOX packs the four u8 values of a sample into one dword the same way and sums them with one v_dot4_u32_u8 against 0x01010101, the + 2
//   as its accumulator.
//   otherwise every group takes the byte path, and so does a last group that holds fewer than 8 pixels.
// Exactly the frame's bytes are written.
template <int FMT, int CHROMA>
__global__ __launch_bounds__(kThreads) void k_ingest_rgb(int w, int h, IngestSrc src, uint8_t *dst, long dst_stride, int groups_x, unsigned n_columns, int wide)
{
    constexpr int bpp = FMT == kPixRgb8 ? 3 : 4;
    const unsigned idx = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (idx >= n_columns) return;
    const int stream = (int)blockIdx.y;
    const int band = (int)(idx / (unsigned)groups_x), x = ((int)idx - band * groups_x) * 8;
    const uint8_t *pic = src.base + (long)stream * src.stride;
    const int cw = w >> 1;
    uint8_t *py = dst + (long)stream * dst_stride, *pu = py + (long)w * h, *pv = pu + (long)cw * (h >> 1);
    const int y_first = band * kIngestPairs * 2;
    if (wide && x + 8 <= w) {
        unsigned r0[kIngestPairs][8], r1[kIngestPairs][8];
#pragma unroll
        for (int j = 0; j < kIngestPairs; j++) {      // every load of the column in flight before the first store
            const int y = y_first + 2 * j;
            if (y >= h) break;
            ingest_load8<FMT>(pic + (long)y * src.pitch + (long)x * bpp, r0[j]);
            ingest_load8<FMT>(pic + (long)(y + 1) * src.pitch + (long)x * bpp, r1[j]);
        }
#pragma unroll
        for (int j = 0; j < kIngestPairs; j++) {
            const int y = y_first + 2 * j;
            if (y >= h) break;
            unsigned ya[2] = {0u, 0u}, yb[2] = {0u, 0u}, uu = 0u, vv = 0u;
#pragma unroll
            for (int c = 0; c < 4; c++) {             // chroma sample c of the group: pixels 2c, 2c + 1 of both rows
                unsigned qu = 0u, qv = 0u;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int k = 2 * c + (i & 1);
                    float r, g, b;
                    ingest_px<FMT>(i < 2 ? r0[j] : r1[j], k, r, g, b);
                    unsigned &yw = i < 2 ? ya[k >> 2] : yb[k >> 2];
                    yw = present_put(ingest_y(r, g, b), k & 3, yw);
                    if (CHROMA == kChromaBox) {
                        qu = present_put(ingest_u(r, g, b), i, qu);
                        qv = present_put(ingest_v(r, g, b), i, qv);
                    } else if (i == 0) {
                        uu = present_put(ingest_u(r, g, b), c, uu);
                        vv = present_put(ingest_v(r, g, b), c, vv);
                    }
                }
                if (CHROMA == kChromaBox) {
                    uu |= (__builtin_amdgcn_udot4(qu, 0x01010101u, 2u, false) >> 2) << (8 * c);
                    vv |= (__builtin_amdgcn_udot4(qv, 0x01010101u, 2u, false) >> 2) << (8 * c);
                }
            }
            st_stream(reinterpret_cast<uint2 *>(py + (long)y * w + x), make_uint2(ya[0], ya[1]));
            st_stream(reinterpret_cast<uint2 *>(py + (long)(y + 1) * w + x), make_uint2(yb[0], yb[1]));
            const long c = (long)(y >> 1) * cw + (x >> 1);
            __builtin_nontemporal_store(uu, reinterpret_cast<unsigned *>(pu + c));
            __builtin_nontemporal_store(vv, reinterpret_cast<unsigned *>(pv + c));
        }
    } else {
        for (int j = 0; j < kIngestPairs; j++) {
            const int y = y_first + 2 * j;
            if (y >= h) break;
            for (int dx = 0; dx < 8 && x + dx < w; dx += 2) ingest_quad_bytes<FMT, CHROMA>(pic, src.pitch, x + dx, y, py, pu, pv, w);
        }
    }
}

}  // namespace pfv
