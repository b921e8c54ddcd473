// pfv_present_kernels.hip -- the last step of a decoder: n_streams planar Y | U | V 4:2:0 frames (packed or padded, where they lie) as
// interleaved RGB8 / RGBA8 / BGRA8 pictures with a row pitch (k_present_rgb).  Arithmetic: include/pfv_hip_ext.h, "RGB / RGBA texture
// output" (normative) -- the reference's save_frame (src/lib.rs:361-394), the expressions of k_yuv420_to_rgb.  A streaming kernel: every
// source byte is read once, every destination byte written once, no atomics, no LDS.
// Included by pfv_capi.hip behind pfv_quality_kernels.hip (SseOperand); the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

constexpr int kPixRgb8 = 0, kPixRgba8 = 1, kPixBgra8 = 2;   // PFV_PIX_* (include/pfv_hip_ext.h)

struct PresentDst {
    uint8_t *base;
    long pitch;      // bytes between the rows of a picture
    long stride;     // bytes between the pictures of consecutive streams
};

// one pixel as its three bytes (R, G, B): JPEG-conversion YCbCr -> RGB in f32, left to right, no contraction, then Rust's `as u8`
__device__ __forceinline__ void present_px(float yy, float u, float v, unsigned &r, unsigned &g, unsigned &b)
{
#pragma clang fp contract(off)
    r = f32_as_u8(yy + (1.402f * v));
    g = f32_as_u8(yy - (0.344136f * u) - (0.714136f * v));
    b = f32_as_u8(yy + (1.772f * u));
}

// The byte-granular path: the 2 x 2 pixels of one chroma sample, byte loads and byte stores.
template <int FMT>
__device__ __forceinline__ void present_quad_bytes(const uint8_t *py, const uint8_t *pu, const uint8_t *pv, int ys, int cs, int x, int y, uint8_t *out,
                                                   long pitch)
{
    constexpr int bpp = FMT == kPixRgb8 ? 3 : 4;
    const long c = (long)(y >> 1) * cs + (x >> 1);
    const float u = (float)pu[c] - 128.0f, v = (float)pv[c] - 128.0f;
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            unsigned r, g, b;
            present_px((float)py[(long)(y + dy) * ys + x + dx], u, v, r, g, b);
            uint8_t *o = out + (long)(y + dy) * pitch + (long)(x + dx) * bpp;
            o[0] = (uint8_t)(FMT == kPixBgra8 ? b : r);
            o[1] = (uint8_t)g;
            o[2] = (uint8_t)(FMT == kPixBgra8 ? r : b);
            if (bpp == 4) o[3] = 255;
        }
}

// The wide path's form of f32_as_u8, with the byte put in its place: v_trunc_f32 truncates toward zero, and v_cvt_pk_u8_f32 -- which on
// its own would round to nearest even -- converts an INTEGRAL value exactly, saturates it to 0 .. 255 (a negative zero included) and
// replaces byte `at` of `word`.  Two instructions per channel instead of convert, compare, select, shift and or; the exhaustive test
// (every Y, U, V triple through this path) holds it equal to f32_as_u8.
__device__ __forceinline__ unsigned present_put(float x, unsigned at, unsigned word)
{
    return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_truncf(x), at, word);
}
// four pixels of one row (luma bytes of `yy`, chroma u / v per pixel pair) as 12 (RGB8) or 16 bytes, one non-temporal store
template <int FMT>
__device__ __forceinline__ void present_row4(uint8_t *out, unsigned yy, const float (&u)[2], const float (&v)[2])
{
#pragma clang fp contract(off)
    float r[4], g[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float y = (float)((yy >> (8 * k)) & 0xffu);
        r[k] = y + (1.402f * v[k >> 1]);
        g[k] = y - (0.344136f * u[k >> 1]) - (0.714136f * v[k >> 1]);
        b[k] = y + (1.772f * u[k >> 1]);
    }
    if (FMT == kPixRgb8) {
        unsigned *o = reinterpret_cast<unsigned *>(out);
        __builtin_nontemporal_store(present_put(r[1], 3, present_put(b[0], 2, present_put(g[0], 1, present_put(r[0], 0, 0u)))), o);
        __builtin_nontemporal_store(present_put(g[2], 3, present_put(r[2], 2, present_put(b[1], 1, present_put(g[1], 0, 0u)))), o + 1);
        __builtin_nontemporal_store(present_put(b[3], 3, present_put(g[3], 2, present_put(r[3], 1, present_put(b[2], 0, 0u)))), o + 2);
    } else {
        unsigned px[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            px[k] = present_put(FMT == kPixBgra8 ? r[k] : b[k], 2, present_put(g[k], 1, present_put(FMT == kPixBgra8 ? b[k] : r[k], 0, 0xff000000u)));
        st_stream(reinterpret_cast<uint4 *>(out), make_uint4(px[0], px[1], px[2], px[3]));
    }
}

constexpr int kPresentPairs = 4;   // row pairs per thread

// One thread owns a column of kPresentPairs groups of 4 x 2 pixels (the index division is paid once for 32 pixels); a group is two luma
// rows and the two chroma samples under them, each chroma sample loaded once for both rows.  Columns are numbered in raster order inside a
// picture (groups_x per band of kPresentPairs row pairs); blockIdx.y is the stream.
//   wide (decided per launch on the host, pfv_present.hip): luma rows, chroma rows and destination rows are all aligned for it.  A lane
//   then loads each luma row as one dword and the chroma of its group as the ALIGNED dword that holds it (two neighbouring lanes share
//   that dword: it is one request to the same line), and stores each row of its group as one 12- or 16-byte non-temporal store; the
//   lanes of a wavefront write one contiguous span of 768 or 1024 bytes per row.  The last group of a row whose width is no multiple
//   of 4 holds 2 pixels: it takes the byte path.
//   otherwise every group takes the byte path.
// Exactly the width x bytes-per-pixel bytes of each row are written.
template <int FMT>
__global__ __launch_bounds__(kThreads) void k_present_rgb(FrameGeom g, SseOperand src, PresentDst dst, int groups_x, unsigned n_columns, int wide)
{
    constexpr int bpp = FMT == kPixRgb8 ? 3 : 4;
    const unsigned idx = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (idx >= n_columns) return;
    const int stream = (int)blockIdx.y;
    const int band = (int)(idx / (unsigned)groups_x), x = ((int)idx - band * groups_x) * 4;
    const uint8_t *frame = src.base + (long)stream * src.stride;
    const uint8_t *py = frame + (src.padded ? g.p[0].pad_off : g.p[0].src_off);
    const uint8_t *pu = frame + (src.padded ? g.p[1].pad_off : g.p[1].src_off);
    const uint8_t *pv = frame + (src.padded ? g.p[2].pad_off : g.p[2].src_off);
    const int ys = src.padded ? g.p[0].pw : g.p[0].w, cs = src.padded ? g.p[1].pw : g.p[1].w;
    uint8_t *out = dst.base + (long)stream * dst.stride;
    const int y_first = band * kPresentPairs * 2, h = g.p[0].h;
    if (wide && x + 4 <= g.p[0].w) {
        const int cx = x >> 1, sh = (cx & 2) * 8;     // the group's two chroma samples: bytes sh / 8 and sh / 8 + 1 of their aligned dword
        unsigned y0[kPresentPairs], y1[kPresentPairs], uu[kPresentPairs], vv[kPresentPairs];
#pragma unroll
        for (int j = 0; j < kPresentPairs; j++) {     // every load of the column in flight before the first store
            const int y = y_first + 2 * j;
            if (y >= h) break;
            const long c = (long)(y >> 1) * cs + (cx & ~3);
            y0[j] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(py + (long)y * ys + x));
            y1[j] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(py + (long)(y + 1) * ys + x));
            uu[j] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(pu + c));
            vv[j] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(pv + c));
        }
#pragma unroll
        for (int j = 0; j < kPresentPairs; j++) {
            const int y = y_first + 2 * j;
            if (y >= h) break;
            float u[2], v[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                u[k] = (float)((uu[j] >> (sh + 8 * k)) & 0xffu) - 128.0f;
                v[k] = (float)((vv[j] >> (sh + 8 * k)) & 0xffu) - 128.0f;
            }
            present_row4<FMT>(out + (long)y * dst.pitch + (long)x * bpp, y0[j], u, v);
            present_row4<FMT>(out + (long)(y + 1) * dst.pitch + (long)x * bpp, y1[j], u, v);
        }
    } else {
        for (int j = 0; j < kPresentPairs; j++) {
            const int y = y_first + 2 * j;
            if (y >= h) break;
            present_quad_bytes<FMT>(py, pu, pv, ys, cs, x, y, out, dst.pitch);
            if (x + 2 < g.p[0].w) present_quad_bytes<FMT>(py, pu, pv, ys, cs, x + 2, y, out, dst.pitch);
        }
    }
}

}  // namespace pfv
