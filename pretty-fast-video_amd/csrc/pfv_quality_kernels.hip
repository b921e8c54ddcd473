// pfv_quality_kernels.hip -- distortion between two frames on the device: squared error per macroblock (k_sse_mb) and per plane
// (k_sse_sum).  Integer arithmetic only; the results do not depend on the launch shape.
// Included by pfv_capi.hip behind pfv_kernels.hip (FrameGeom, locate_strip, mb_sum); the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

// One of the two frames that are compared: n_streams frames `stride` bytes apart, each Y | U | V in one of the two layouts the project
// uses -- packed (plane stride = plane width, PlaneGeom::src_off) or padded (plane stride = pad16(width), PlaneGeom::pad_off).
struct SseOperand {
    const uint8_t *base;
    long stride;     // bytes between the frames of consecutive streams
    int padded;      // 0: packed frame, 1: padded frame
    int vec;         // bit p: 16-byte loads of plane p are legal (plane base and row stride 16-byte aligned for every stream)
};

// 16 bytes (x .. x + 15 of row y) of one plane, of which the first n lie inside the picture (w x h); a row below the picture reads as 0.
// A padded row holds pad16(w) bytes, so its last 16-byte segment may be loaded whole; a packed row is only loaded whole when all 16
// pixels belong to it.  The vector form returns the bytes as they lie: the caller masks those beyond n (sse_mask) AFTER all its loads
// have been issued, so that no load waits for the one before it.
__device__ __forceinline__ uint4 sse_load16(const SseOperand &o, const uint8_t *plane, int row_stride, bool vec, int x, int y, int n, int h)
{
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if (y >= h || n <= 0) return val;
    const uint8_t *src = plane + (long)y * row_stride + x;
    if (vec && (n == 16 || o.padded)) {
        val = *reinterpret_cast<const uint4 *>(src);
    } else {
        unsigned wds[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            unsigned acc = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (i * 4 + b < n) acc |= (unsigned)src[i * 4 + b] << (8 * b);
            wds[i] = acc;
        }
        val = make_uint4(wds[0], wds[1], wds[2], wds[3]);
    }
    return val;
}
// dword i of a 16-byte segment with only its first n bytes inside the picture: the bytes that count
__device__ __forceinline__ unsigned sse_mask(int n, int i)
{
    const int k = n - 4 * i;
    return k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : (1u << (8 * k)) - 1u);
}

// sum of a^2, b^2 and ab over 16 pixels: per lane and launch at most 32 x 255^2 = 2 080 800 each (below 2^23)
__device__ __forceinline__ void sse_dots(const uint4 &a, const uint4 &b, unsigned &aa, unsigned &bb, unsigned &ab)
{
    aa = __builtin_amdgcn_udot4(a.w, a.w, __builtin_amdgcn_udot4(a.z, a.z, __builtin_amdgcn_udot4(a.y, a.y, __builtin_amdgcn_udot4(a.x, a.x, aa, false), false), false), false);
    bb = __builtin_amdgcn_udot4(b.w, b.w, __builtin_amdgcn_udot4(b.z, b.z, __builtin_amdgcn_udot4(b.y, b.y, __builtin_amdgcn_udot4(b.x, b.x, bb, false), false), false), false);
    ab = __builtin_amdgcn_udot4(a.w, b.w, __builtin_amdgcn_udot4(a.z, b.z, __builtin_amdgcn_udot4(a.y, b.y, __builtin_amdgcn_udot4(a.x, b.x, ab, false), false), false), false);
}

// Squared error per macroblock: mb_sse[stream][macroblock], macroblocks in frame order (Y, U, V; raster inside a plane) -- the index
// space of mv / has_coef.  The project's mapping: one wavefront per strip of 8 macroblocks, lane (m, i) owns rows i and i + 8 of
// macroblock m.  A lane's sum(a^2) + sum(b^2) - 2 sum(ab) is the complete squared error of ITS 32 pixels, so it is never negative and
// stays below 2^22; a macroblock's total is at most 256 x 255^2 = 16 646 400.  Every macroblock of the frame is written: nothing has to
// be cleared beforehand.
__global__ __launch_bounds__(kThreads) void k_sse_mb(FrameGeom g, SseOperand A, SseOperand B, uint32_t *__restrict__ mb_sse)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gstrip = (int)blockIdx.x * kStripsPerWG + wave;
    if (gstrip >= g.strips_per_frame * g.n_streams) return;   // no cross-wavefront sync in this kernel
    const StripPos sp = locate_strip(g, gstrip);
    const PlaneGeom &p = g.p[sp.plane];
    const int m = lane >> 3, i = lane & 7;
    const uint8_t *pa = A.base + (long)sp.stream * A.stride + (A.padded ? p.pad_off : p.src_off);
    const uint8_t *pb = B.base + (long)sp.stream * B.stride + (B.padded ? p.pad_off : p.src_off);
    const int sa = A.padded ? p.pw : p.w, sb = B.padded ? p.pw : p.w;
    const bool va = (A.vec >> sp.plane) & 1, vb = (B.vec >> sp.plane) & 1;
    const int x = sp.x0 + m * 16, n = min(16, p.w - x);   // n: pixels of the lane's segments inside the picture (<= 0: none)
    uint4 ra[2], rb[2];
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {   // all four loads in flight before the first dot
        ra[pass] = sse_load16(A, pa, sa, va, x, sp.y0 + i + 8 * pass, n, p.h);
        rb[pass] = sse_load16(B, pb, sb, vb, x, sp.y0 + i + 8 * pass, n, p.h);
    }
    const uint4 mk = make_uint4(sse_mask(n, 0), sse_mask(n, 1), sse_mask(n, 2), sse_mask(n, 3));
    unsigned aa = 0, bb = 0, ab = 0;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const uint4 a = make_uint4(ra[pass].x & mk.x, ra[pass].y & mk.y, ra[pass].z & mk.z, ra[pass].w & mk.w);
        const uint4 b = make_uint4(rb[pass].x & mk.x, rb[pass].y & mk.y, rb[pass].z & mk.z, rb[pass].w & mk.w);
        sse_dots(a, b, aa, bb, ab);
    }
    const int total = mb_sum((int)(aa + bb - 2u * ab));
    if (i == 0 && m < sp.n_mb) mb_sse[(long)sp.stream * g.mbs_per_frame + sp.mb_first + m] = (uint32_t)total;
}

// The map summed per (stream, plane) into sse[stream][3]: one workgroup each, every thread a strided share of the plane's
// macroblocks, wave reduction, LDS, one 64-bit store.  No atomics and nothing to clear: the pair k_sse_mb + k_sse_sum gives the same
// numbers for any arrival order and can be recorded in a graph as two kernel nodes.
__global__ __launch_bounds__(kThreads) void k_sse_sum(FrameGeom g, const uint32_t *__restrict__ mb_sse, uint64_t *__restrict__ sse)
{
    __shared__ unsigned long long part[kStripsPerWG];
    const int stream = (int)blockIdx.x / 3, plane = (int)blockIdx.x - stream * 3;
    const PlaneGeom &p = g.p[plane];
    const uint32_t *src = mb_sse + (long)stream * g.mbs_per_frame + p.mb0;
    const int n = p.bw * p.bh;
    unsigned long long acc = 0;
    for (int k = threadIdx.x; k < n; k += kThreads) acc += src[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)acc, off), hi = (unsigned)__shfl_xor((int)(unsigned)(acc >> 32), off);
        acc += ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < kStripsPerWG; w++) total += part[w];
        sse[(long)stream * 3 + plane] = total;
    }
}

}  // namespace pfv
