// pfv_ssim_kernels.hip -- structural similarity between two frames on the device, in the integer form of the common video tools: 8 x 8 windows
// at stride 4 built from 4 x 4 block sums, one value per window in 2^-24 fixed point, summed per macroblock (k_ssim_mb) and per plane
// (k_ssim_sum).  The four sums of a window are exact integers; only the final quotient is f32.  No atomics: the sums are integers, so the
// results do not depend on the launch shape or the arrival order.  The definition is normative in include/pfv_hip_ext.h.
// Included by pfv_capi.hip behind pfv_quality_kernels.hip (SseOperand, sse_load16); the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

constexpr int kSsimC1 = 416;        // (0.01 * 255)^2 * 64, rounded
constexpr int kSsimC2 = 235963;     // (0.03 * 255)^2 * 64 * 63, rounded
constexpr int kQuadReverse = 0x1B;  // quad_perm:[3,2,1,0]

// the block column to the right of a lane's 16-byte segment (x .. x + 3 of row y, of which the first k lie inside the picture) for the lanes
// that have no neighbouring macroblock in their wavefront; reads as nothing below and beside the picture, like sse_load16
__device__ __forceinline__ unsigned ssim_load4(const SseOperand &o, const uint8_t *plane, int row_stride, bool vec, int x, int y, int k, int h)
{
    if (y >= h || k <= 0) return 0u;
    const uint8_t *src = plane + (long)y * row_stride + x;
    if (vec && (k >= 4 || o.padded)) return *reinterpret_cast<const unsigned *>(src);
    unsigned acc = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (b < k) acc |= (unsigned)src[b] << (8 * b);
    return acc;
}

// sum over the four lanes of a quad: the four rows of a block row
__device__ __forceinline__ int quad_sum(int v)
{
    v += dpp<kQuadXor1>(v);
    v += dpp<kQuadXor2>(v);
    return v;
}
// the value of lane i ^ 4: the other quad of the macroblock's eight lanes
__device__ __forceinline__ int other_quad(int v) { return dpp<kQuadReverse>(dpp<kRowHalfMirror>(v)); }

// The sums of one row of five blocks, per pair of neighbouring blocks (the width of a window), then over the rows of the quad; pair j is
// left in lane j of the quad.  s holds sum(a) in its low and sum(b) in its high half: a window's are at most 64 x 255 = 16 320 each.
struct SsimSums { int s, ss, s12; };
__device__ __forceinline__ SsimSums ssim_block_row(const uint4 &a, unsigned a4, const uint4 &b, unsigned b4, int j)
{
    const unsigned av[5] = {a.x, a.y, a.z, a.w, a4}, bv[5] = {b.x, b.y, b.z, b.w, b4};
    unsigned s[5], ss[5], s12[5];
#pragma unroll
    for (int d = 0; d < 5; d++) {   // a dword of a row is one block-row
        s[d] = __builtin_amdgcn_udot4(av[d], 0x01010101u, __builtin_amdgcn_udot4(bv[d], 0x01010101u, 0u, false) << 16, false);
        ss[d] = __builtin_amdgcn_udot4(av[d], av[d], __builtin_amdgcn_udot4(bv[d], bv[d], 0u, false), false);
        s12[d] = __builtin_amdgcn_udot4(av[d], bv[d], 0u, false);
    }
    SsimSums pair[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        pair[d].s = quad_sum((int)(s[d] + s[d + 1]));
        pair[d].ss = quad_sum((int)(ss[d] + ss[d + 1]));
        pair[d].s12 = quad_sum((int)(s12[d] + s12[d + 1]));
    }
    const SsimSums lo = (j & 1) ? pair[1] : pair[0], hi = (j & 1) ? pair[3] : pair[2];
    return (j & 2) ? hi : lo;
}
__device__ __forceinline__ SsimSums operator+(const SsimSums &x, const SsimSums &y) { return SsimSums{x.s + y.s, x.ss + y.ss, x.s12 + y.s12}; }

// One window from its four sums over 64 pixels.  s1^2 + s2^2 <= 2 x 16 320^2 and 64 ss <= 64 x 64 x 2 x 255^2 are both 532 684 800: every
// integer below stays under 2^30.  The quotient is IEEE single precision with a true division; |ssim| <= 1, so q fits 2^24 in magnitude.
__device__ __forceinline__ int ssim_window_q24(const SsimSums &w)
{
    const int s1 = w.s & 0xffff, s2 = (int)((unsigned)w.s >> 16);
    const int sq = s1 * s1 + s2 * s2, cross = s1 * s2;
    const int vars = 64 * w.ss - sq, covar = 64 * w.s12 - cross;
    const float num = (float)(2 * cross + kSsimC1) * (float)(2 * covar + kSsimC2);
    const float den = (float)(sq + kSsimC1) * (float)(vars + kSsimC2);
    return (int)__builtin_rintf((num / den) * 16777216.0f);
}

// SSIM per macroblock: mb_ssim[stream][macroblock] = the sum of q over the windows whose top-left pixel lies in the macroblock, macroblocks in
// the index space of mv / has_coef.  The project's mapping: one wavefront per strip of 8 macroblocks, lane (m, i) owns rows i and i + 8 of
// macroblock m.  The 16 windows of a macroblock need 5 x 5 blocks.  The fifth block column is the first dword of the macroblock to the right:
// from lane (m + 1, i), or loaded for the last macroblock of the strip.  The fifth block row is rows 16..19, which belong to the strip below:
// a third pass in which both quads load row 16 + (i & 3).  After the sums over a quad, lane (j, quad) holds column pair j of block rows quad,
// quad + 2 and 4; one exchange with the other quad gives it two vertically neighbouring windows.  A window exists when both its block columns
// and both its block rows do (w >> 2, h >> 2 whole blocks): all its 64 pixels then lie inside the picture.  So the bytes beyond the picture
// that an aligned load of a padded row brings along (k_sse_mb masks them, sse_mask) only ever reach windows that do not exist, and no mask is
// needed; they are bytes like any other, so the integer bounds hold for those windows too.  Every macroblock of the frame is written.
__global__ __launch_bounds__(kThreads) void k_ssim_mb(FrameGeom g, SseOperand A, SseOperand B, int32_t *__restrict__ mb_ssim)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gstrip = (int)blockIdx.x * kStripsPerWG + wave;
    if (gstrip >= g.strips_per_frame * g.n_streams) return;   // no cross-wavefront sync in this kernel
    const StripPos sp = locate_strip(g, gstrip);
    const PlaneGeom &p = g.p[sp.plane];
    const int m = lane >> 3, i = lane & 7, quad = i >> 2, j = i & 3;
    const uint8_t *pa = A.base + (long)sp.stream * A.stride + (A.padded ? p.pad_off : p.src_off);
    const uint8_t *pb = B.base + (long)sp.stream * B.stride + (B.padded ? p.pad_off : p.src_off);
    const int sa = A.padded ? p.pw : p.w, sb = B.padded ? p.pw : p.w;
    const bool va = (A.vec >> sp.plane) & 1, vb = (B.vec >> sp.plane) & 1;
    const int x = sp.x0 + m * 16, left = p.w - x, n = min(16, left);   // left: pixels of the picture from the lane's segment on (<= 0: none)
    const int row[3] = {sp.y0 + i, sp.y0 + i + 8, sp.y0 + 16 + j};
    const bool last = m == kStripMB - 1;
    SsimSums h[3];
#pragma unroll
    for (int pass = 0; pass < 3; pass++) {
        const uint4 a = sse_load16(A, pa, sa, va, x, row[pass], n, p.h), b = sse_load16(B, pb, sb, vb, x, row[pass], n, p.h);
        const unsigned ea = last ? ssim_load4(A, pa, sa, va, x + 16, row[pass], left - 16, p.h) : 0u;
        const unsigned eb = last ? ssim_load4(B, pb, sb, vb, x + 16, row[pass], left - 16, p.h) : 0u;
        const unsigned na = (unsigned)__shfl((int)a.x, (lane + 8) & 63), nb = (unsigned)__shfl((int)b.x, (lane + 8) & 63);
        h[pass] = ssim_block_row(a, last ? ea : na, b, last ? eb : nb, j);
    }
    // quad 0 holds block rows 0, 2, 4 and takes the windows of rows 0 and 1; quad 1 holds 1, 3, 4 and takes rows 2 and 3
    const SsimSums send = quad ? h[0] : h[1];
    const SsimSums got = SsimSums{other_quad(send.s), other_quad(send.ss), other_quad(send.s12)};
    const SsimSums win0 = got + (quad ? h[1] : h[0]), win1 = h[1] + (quad ? h[2] : got);
    const int bx = (x >> 2) + j, by = (sp.y0 >> 2) + 2 * quad;
    int q = 0;
    if (bx + 1 < (p.w >> 2)) {
        if (by + 1 < (p.h >> 2)) q += ssim_window_q24(win0);
        if (by + 2 < (p.h >> 2)) q += ssim_window_q24(win1);
    }
    const int total = mb_sum(q);   // at most 16 windows: |total| <= 2^28
    if (i == 0 && m < sp.n_mb) mb_ssim[(long)sp.stream * g.mbs_per_frame + sp.mb_first + m] = total;
}

// The map summed per (stream, plane) into ssim[stream][3]: the form of k_sse_sum, signed.
__global__ __launch_bounds__(kThreads) void k_ssim_sum(FrameGeom g, const int32_t *__restrict__ mb_ssim, int64_t *__restrict__ ssim)
{
    __shared__ long long part[kStripsPerWG];
    const int stream = (int)blockIdx.x / 3, plane = (int)blockIdx.x - stream * 3;
    const PlaneGeom &p = g.p[plane];
    const int32_t *src = mb_ssim + (long)stream * g.mbs_per_frame + p.mb0;
    const int n = p.bw * p.bh;
    long long acc = 0;
    for (int k = threadIdx.x; k < n; k += kThreads) acc += src[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {   // two's complement: the halves travel as bits
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)acc, off);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)acc >> 32), off);
        acc = (long long)((unsigned long long)acc + (((unsigned long long)hi << 32) | lo));
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long total = 0;
#pragma unroll
        for (int w = 0; w < kStripsPerWG; w++) total += part[w];
        ssim[(long)stream * 3 + plane] = total;
    }
}

}  // namespace pfv
