// pfv_deblock_kernels.hip -- out-of-loop deblocking of the frames that are shown (k_deblock): the two-stage integer filter over the 8 x 8 transform
// grid of each plane that include/pfv_hip_ext.h defines ("out-of-loop deblocking", normative).  It reads a frame (packed or padded) and writes a
// packed one; the framebuffer a p-frame predicts from is never its destination.  Integer arithmetic only, no atomics; edges of one stage touch
// disjoint samples, so the result does not depend on the launch shape.
// Included by pfv_capi.hip behind pfv_ssim_kernels.hip (SseOperand, sse_load16, ssim_load4); the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

constexpr int kDeblockMaxS = 12;
constexpr int kDbRows = 20;                   // rows a macroblock's lanes exchange: its own 16, then y0 - 2, y0 - 1, y0 + 16, y0 + 17
constexpr int kDbPitch = kDbRows * 4 + 4;     // dwords per macroblock; the 4 spare dwords keep the eight macroblocks off each other's banks

struct DeblockStrength { int s[3]; };         // per plane, 0 .. kDeblockMaxS

// One edge between B and C of the line A B | C D, strength S.  tdiv truncates toward zero: the bias makes the arithmetic shift do so.
__device__ __forceinline__ void deblock_edge(int &A, int &B, int &C, int &D, int S)
{
    const int t = A - 4 * B + 4 * C - D;
    const int d = (t + ((t >> 31) & 7)) >> 3;
    const int ad = d < 0 ? -d : d;
    const int m = max(0, ad - max(0, 2 * (ad - S)));     // ramps up to S, back to 0 at 2S
    const int d1 = d < 0 ? -m : m;
    const int u = A - D;
    const int lim = m >> 1;
    const int d2 = min(max((u + ((u >> 31) & 3)) >> 2, -lim), lim);
    B = min(max(B + d1, 0), 255);
    C = min(max(C - d1, 0), 255);
    A -= d2;     // A and D move toward each other by at most |A - D| / 4: no clamp
    D += d2;
}
__device__ __forceinline__ int db_byte(unsigned v, int k) { return (int)((v >> (8 * k)) & 0xffu); }

// Stage 1 on the 16 bytes x .. x + 15 of one row: the interior edge at x + 8, and the lane's own bytes of the two edges it shares with the
// segments beside it -- left holds bytes x - 4 .. x - 1, right bytes x + 16 .. x + 19.  e0 / e1 / e2: the edge at x / x + 8 / x + 16 exists.
// Every edge is computed from the INPUT row (the edges are 8 apart and reach +-2: their samples are disjoint).
__device__ __forceinline__ uint4 deblock_row(const uint4 &v, unsigned left, unsigned right, bool e0, bool e1, bool e2, int S)
{
    uint4 out = v;
    {
        int A = db_byte(left, 2), B = db_byte(left, 3), C = db_byte(v.x, 0), D = db_byte(v.x, 1);
        deblock_edge(A, B, C, D, S);
        if (e0) out.x = (v.x & 0xffff0000u) | (unsigned)C | ((unsigned)D << 8);
    }
    {
        int A = db_byte(v.y, 2), B = db_byte(v.y, 3), C = db_byte(v.z, 0), D = db_byte(v.z, 1);
        deblock_edge(A, B, C, D, S);
        if (e1) {
            out.y = (v.y & 0x0000ffffu) | ((unsigned)A << 16) | ((unsigned)B << 24);
            out.z = (v.z & 0xffff0000u) | (unsigned)C | ((unsigned)D << 8);
        }
    }
    {
        int A = db_byte(v.w, 2), B = db_byte(v.w, 3), C = db_byte(right, 0), D = db_byte(right, 1);
        deblock_edge(A, B, C, D, S);
        if (e2) out.w = (v.w & 0x0000ffffu) | ((unsigned)A << 16) | ((unsigned)B << 24);
    }
    return out;
}

// two neighbouring columns of one exchanged row (2 bytes at an even offset)
__device__ __forceinline__ unsigned db_get2(const unsigned *mb, int row, int col)
{
    return (mb[row * 4 + (col >> 2)] >> (8 * (col & 2))) & 0xffffu;
}

// The project's mapping (k_sse_mb, k_ssim_mb): one wavefront per strip of 8 macroblocks, lane (m, i) owns rows i and i + 8 of macroblock m as
// 16-byte vectors, and writes exactly those.
//   Stage 1 (vertical edges) is local to a row.  The bytes beside a segment come from lanes +-8 (the macroblocks beside it) and, at the first
//   and last macroblock of the strip, from a 4-byte load.
//   Stage 2 (horizontal edges at y0, y0 + 8, y0 + 16) works on the stage-1 result and needs the four rows y0 - 2, y0 - 1, y0 + 16, y0 + 17 of
//   the strips above and below: a third pass in which the first quad loads the row of lane i & 3 and runs stage 1 on it.  The 20 rows of a
//   macroblock then meet in the wavefront's own LDS region; lane i filters columns 2i and 2i + 1 of all three edges there (of the edge at y0
//   only the rows below it are the strip's own, of the one at y0 + 16 only the rows above it), and every lane reads its two rows back.
// An edge exists only where all four of its samples lie inside w x h, so bytes beyond the picture (the zeros sse_load16 returns, or what a
// whole load of a padded row brings along) never reach a sample that is stored.  S == 0 copies: a wave-uniform short cut.
__global__ __launch_bounds__(kThreads) void k_deblock(FrameGeom g, SseOperand src, uint8_t *__restrict__ dst, long dst_stride, int dst_vec,
                                                       DeblockStrength strength)
{
    __shared__ __attribute__((aligned(16))) unsigned xrows[kStripsPerWG][kStripMB * kDbPitch];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gstrip = xcd_remap((int)blockIdx.x, (int)gridDim.x) * kStripsPerWG + wave;
    if (gstrip >= g.strips_per_frame * g.n_streams) return;   // no cross-wavefront sync in this kernel
    const StripPos sp = locate_strip(g, gstrip);
    const PlaneGeom &p = g.p[sp.plane];
    const int m = lane >> 3, i = lane & 7, j = i & 3;
    const uint8_t *ps = src.base + (long)sp.stream * src.stride + (src.padded ? p.pad_off : p.src_off);
    uint8_t *pd = dst + (long)sp.stream * dst_stride + p.src_off;
    const int ss = src.padded ? p.pw : p.w;
    const bool vs = (src.vec >> sp.plane) & 1, vd = (dst_vec >> sp.plane) & 1;
    const int S = sp.plane == 0 ? strength.s[0] : (sp.plane == 1 ? strength.s[1] : strength.s[2]);
    const int x = sp.x0 + m * 16, left = p.w - x, n = min(16, left);   // left: pixels of the picture from the lane's segment on (<= 0: none)
    const int halo = j < 2 ? sp.y0 - 2 + j : sp.y0 + 14 + j;
    const int row[3] = {sp.y0 + i, sp.y0 + i + 8, (halo < 0 || i >= 4) ? p.h : halo};   // a row above the picture reads as one below it: nothing; the second quad has no halo row
    uint4 r[3];
    if (S == 0) {
        r[0] = sse_load16(src, ps, ss, vs, x, row[0], n, p.h);
        r[1] = sse_load16(src, ps, ss, vs, x, row[1], n, p.h);
    } else {
        const bool first = m == 0, last = m == kStripMB - 1;
        const bool e0 = x >= 8 && x + 1 < p.w, e1 = x + 9 < p.w, e2 = x + 17 < p.w;
        uint4 v[3];
        unsigned el[3], er[3];
#pragma unroll
        for (int pass = 0; pass < 3; pass++) {   // every load in flight before the first edge
            v[pass] = sse_load16(src, ps, ss, vs, x, row[pass], n, p.h);
            el[pass] = (first && x > 0) ? ssim_load4(src, ps, ss, vs, x - 4, row[pass], 4, p.h) : 0u;
            er[pass] = last ? ssim_load4(src, ps, ss, vs, x + 16, row[pass], left - 16, p.h) : 0u;
        }
#pragma unroll
        for (int pass = 0; pass < 3; pass++) {
            const unsigned nl = (unsigned)__shfl((int)v[pass].w, (lane - 8) & 63), nr = (unsigned)__shfl((int)v[pass].x, (lane + 8) & 63);
            r[pass] = deblock_row(v[pass], first ? el[pass] : nl, last ? er[pass] : nr, e0, e1, e2, S);
        }
        // stage 2 in the wavefront's LDS region
        unsigned *mb = &xrows[wave][m * kDbPitch];
        *reinterpret_cast<uint4 *>(mb + i * 4) = r[0];
        *reinterpret_cast<uint4 *>(mb + (i + 8) * 4) = r[1];
        if (i < 4) *reinterpret_cast<uint4 *>(mb + (16 + j) * 4) = r[2];
        wave_lds_sync();
        const int c = 2 * i, dw = c >> 2, sh = 8 * (c & 2);
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const int ye = sp.y0 + 8 * e;
            if (ye < 8 || ye + 1 >= p.h) continue;   // wave-uniform
            const int ra = e == 0 ? 16 : (e == 1 ? 6 : 14), rb = ra + 1, rc = e == 0 ? 0 : (e == 1 ? 8 : 18), rd = rc + 1;
            const unsigned a2 = db_get2(mb, ra, c), b2 = db_get2(mb, rb, c), c2 = db_get2(mb, rc, c), d2 = db_get2(mb, rd, c);
            unsigned oa = 0, ob = 0, oc = 0, od = 0;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                int A = db_byte(a2, k), B = db_byte(b2, k), C = db_byte(c2, k), D = db_byte(d2, k);
                deblock_edge(A, B, C, D, S);
                oa |= (unsigned)A << (8 * k); ob |= (unsigned)B << (8 * k); oc |= (unsigned)C << (8 * k); od |= (unsigned)D << (8 * k);
            }
            // a dword of a row is shared by two lanes (columns 2i, 2i + 1 are half of it): each rewrites only its own half, as 16-bit stores
            uint16_t *h = reinterpret_cast<uint16_t *>(mb);
            if (e != 0) {
                h[(ra * 4 + dw) * 2 + (sh >> 4)] = (uint16_t)oa;
                h[(rb * 4 + dw) * 2 + (sh >> 4)] = (uint16_t)ob;
            }
            if (e != 2) {
                h[(rc * 4 + dw) * 2 + (sh >> 4)] = (uint16_t)oc;
                h[(rd * 4 + dw) * 2 + (sh >> 4)] = (uint16_t)od;
            }
        }
        wave_lds_sync();
        r[0] = *reinterpret_cast<const uint4 *>(mb + i * 4);
        r[1] = *reinterpret_cast<const uint4 *>(mb + (i + 8) * 4);
    }
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int y = row[pass];
        if (y >= p.h || n <= 0) continue;
        uint8_t *out = pd + (long)y * p.w + x;
        if (vd && n == 16) {
            *reinterpret_cast<uint4 *>(out) = r[pass];
        } else {
            const unsigned wds[4] = {r[pass].x, r[pass].y, r[pass].z, r[pass].w};
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (b < n) out[b] = (uint8_t)(wds[b >> 2] >> (8 * (b & 3)));
        }
    }
}

}  // namespace pfv
