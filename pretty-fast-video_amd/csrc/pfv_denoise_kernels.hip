// pfv_denoise_kernels.hip -- spatio-temporal noise filter ahead of the encoder (k_denoise): the two-stage integer filter that
// include/pfv_hip_ext.h defines ("denoising pre-filter", normative).  Stage 1 is a 3 x 3 ramp-limited smoothing of the input plane, stage 2 a
// ramp-limited step toward the stream's previous output (the state).  It reads a frame (packed or padded), writes a packed one and, when the
// run commits, the state in place.  Integer arithmetic only, no atomics; stage 1 reads only the input and stage 2 is pointwise, so the result
// does not depend on the launch shape.
// Included by pfv_capi.hip behind pfv_ssim_kernels.hip (SseOperand, sse_load16, ssim_load4); the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

constexpr int kDenoiseMaxS = 16;

struct DenoiseStrength { int ss[3], st[3]; };   // per plane: spatial, temporal; 0 .. kDenoiseMaxS

// Two samples side by side as 16-bit integers: every value of the filter fits (differences +-255, the weighted sum of twelve ramps +-192), and
// gfx950 evaluates both halves in one packed instruction (v_pk_sub_i16, v_pk_min_i16, v_pk_max_i16, v_pk_add_i16, v_pk_ashrrev_i16).  A plain
// compiler vector: the emulator build takes the same source.
typedef short pk16 __attribute__((vector_size(4)));
__device__ __forceinline__ pk16 pk_of(unsigned u) { pk16 r; __builtin_memcpy(&r, &u, 4); return r; }
__device__ __forceinline__ unsigned pk_bits(pk16 v) { unsigned u; __builtin_memcpy(&u, &v, 4); return u; }
__device__ __forceinline__ pk16 pk_splat(int v) { const pk16 r = {(short)v, (short)v}; return r; }
__device__ __forceinline__ pk16 pk_min(pk16 a, pk16 b) { return a < b ? a : b; }
__device__ __forceinline__ pk16 pk_max(pk16 a, pk16 b) { return a > b ? a : b; }

// phi(d, S) = sign(d) * max(0, min(|d|, 2S - |d|)) without the sign and the absolute value: for d >= 0 only the first term is non-zero, for
// d < 0 only the second.  s2 = 2S, ns2 = -2S.  |d| beyond 2S gives 0, which is what an "outside" neighbour (kDnOutside) relies on.
__device__ __forceinline__ pk16 dn_phi(pk16 d, pk16 s2, pk16 ns2)
{
    const pk16 zero = pk_splat(0);
    return pk_max(pk_min(d, s2 - d), zero) + pk_min(pk_max(d, ns2 - d), zero);
}

// A neighbour outside w x h contributes 0: its 16-bit value carries this bit, so that its difference to any sample is at least 16129 > 2S.
constexpr unsigned kDnOutside = 0x4000u;

// One row of a lane, ready for the filter: for dword k (bytes b0 .. b3 at columns 4k .. 4k + 3) the pairs
//   e = (b0, b2)   o = (b1, b3)   l = (b-1, b1)   r = (b2, b4)
// so that e's left / right neighbours are l / o and o's are e / r.
struct DnRow { unsigned e[4], o[4], l[4], r[4]; };

// v: the 16 bytes; lb / rb: the dwords that hold column x - 1 in byte 3 / column x + 16 in byte 0; the marks flag pairs outside the picture
__device__ __forceinline__ void dn_unpack(DnRow &R, const uint4 &v, unsigned lb, unsigned rb, const DnRow &mark, unsigned rowmark)
{
    const unsigned w[6] = {lb, v.x, v.y, v.z, v.w, rb};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned c = w[k + 1];
        R.e[k] = (c & 0x00ff00ffu) | mark.e[k] | rowmark;
        R.o[k] = ((c >> 8) & 0x00ff00ffu) | mark.o[k] | rowmark;
        R.l[k] = (__builtin_amdgcn_alignbyte(c, w[k], 3) & 0x00ff00ffu) | mark.l[k] | rowmark;
        R.r[k] = ((__builtin_amdgcn_alignbyte(w[k + 2], c, 1) >> 8) & 0x00ff00ffu) | mark.r[k] | rowmark;
    }
}

// stage 1 for the pair c with its eight neighbours: edge neighbours weigh 2, diagonal ones 1
__device__ __forceinline__ pk16 dn_spatial(pk16 c, unsigned up_l, unsigned up_c, unsigned up_r, unsigned left, unsigned right, unsigned dn_l, unsigned dn_c,
                                           unsigned dn_r, pk16 s2, pk16 ns2)
{
    const pk16 edge = dn_phi(pk_of(up_c) - c, s2, ns2) + dn_phi(pk_of(left) - c, s2, ns2) + dn_phi(pk_of(right) - c, s2, ns2) + dn_phi(pk_of(dn_c) - c, s2, ns2);
    const pk16 diag = dn_phi(pk_of(up_l) - c, s2, ns2) + dn_phi(pk_of(up_r) - c, s2, ns2) + dn_phi(pk_of(dn_l) - c, s2, ns2) + dn_phi(pk_of(dn_r) - c, s2, ns2);
    return c + ((edge + edge + diag + pk_splat(8)) >> pk_splat(4));
}

// stage 2: s + tdiv(3 * phi(P - s, St), 4); the bias makes the arithmetic shift truncate toward zero
__device__ __forceinline__ pk16 dn_temporal(pk16 s, pk16 P, pk16 t2, pk16 nt2)
{
    const pk16 f = dn_phi(P - s, t2, nt2);
    const pk16 t = f + f + f;
    return s + ((t + ((t >> pk_splat(15)) & pk_splat(3))) >> pk_splat(2));
}

// the row of lane i - 1 / i + 1 of the macroblock's eight lanes, wrapping around inside them
__device__ __forceinline__ void dn_ring(const uint4 &v, unsigned lr, int prev, int next, uint4 &pv, unsigned &plr, uint4 &nv, unsigned &nlr)
{
    pv = make_uint4((unsigned)__shfl((int)v.x, prev), (unsigned)__shfl((int)v.y, prev), (unsigned)__shfl((int)v.z, prev), (unsigned)__shfl((int)v.w, prev));
    nv = make_uint4((unsigned)__shfl((int)v.x, next), (unsigned)__shfl((int)v.y, next), (unsigned)__shfl((int)v.z, next), (unsigned)__shfl((int)v.w, next));
    plr = (unsigned)__shfl((int)lr, prev);
    nlr = (unsigned)__shfl((int)lr, next);
}

// The mapping of k_deblock: one wavefront per strip of 8 macroblocks, lane (m, i) owns rows i and i + 8 of macroblock m as 16-byte vectors, and
// writes exactly those.
//   Columns x - 1 and x + 16 come from lanes -+8 (the macroblocks beside it) and, at the first and last macroblock of the strip, from a 4-byte load.
//   Rows i +- 1 and i + 8 +- 1 are the registers of the lanes i +- 1 (row i + 8 of lane 7 lies above row i of lane 0's second row, and so on); the
//   two halo rows y0 - 1 and y0 + 16 are a third load, by lanes i == 0 and i == 7.
// A neighbour exists only inside w x h: a pair outside carries kDnOutside, so bytes beyond the picture (the zeros sse_load16 returns, or what a
// whole load of a padded row brings along) never reach a sample that is stored.  Ss == 0 skips stage 1, St == 0 or an unprimed stream stage 2:
// wave-uniform short cuts.  `primed` and `state` are those of the launch's first stream.
__global__ __launch_bounds__(kThreads) void k_denoise(FrameGeom g, SseOperand src, uint8_t *__restrict__ dst, long dst_stride, int dst_vec,
                                                       uint8_t *__restrict__ state, int state_vec, const uint32_t *__restrict__ primed, DenoiseStrength strength,
                                                       int commit)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gstrip = xcd_remap((int)blockIdx.x, (int)gridDim.x) * kStripsPerWG + wave;
    if (gstrip >= g.strips_per_frame * g.n_streams) return;   // no cross-wavefront sync in this kernel
    const StripPos sp = locate_strip(g, gstrip);
    const PlaneGeom &p = g.p[sp.plane];
    const int m = lane >> 3, i = lane & 7;
    const uint8_t *ps = src.base + (long)sp.stream * src.stride + (src.padded ? p.pad_off : p.src_off);
    uint8_t *pd = dst + (long)sp.stream * dst_stride + p.src_off;
    uint8_t *pt = state + (long)sp.stream * g.src_frame_bytes + p.src_off;
    const int ss = src.padded ? p.pw : p.w;
    const bool vs = (src.vec >> sp.plane) & 1, vd = (dst_vec >> sp.plane) & 1, vt = (state_vec >> sp.plane) & 1;
    const int Ss = sp.plane == 0 ? strength.ss[0] : (sp.plane == 1 ? strength.ss[1] : strength.ss[2]);
    const int St = sp.plane == 0 ? strength.st[0] : (sp.plane == 1 ? strength.st[1] : strength.st[2]);
    const bool temporal = St != 0 && primed[sp.stream] != 0;   // wave-uniform
    const int x = sp.x0 + m * 16, left = p.w - x, n = min(16, left);   // left: pixels of the picture from the lane's segment on (<= 0: none)
    const int row[2] = {sp.y0 + i, sp.y0 + i + 8};
    const SseOperand sto = {state, g.src_frame_bytes, 0, state_vec};
    uint4 r[2];
    r[0] = sse_load16(src, ps, ss, vs, x, row[0], n, p.h);
    r[1] = sse_load16(src, ps, ss, vs, x, row[1], n, p.h);
    uint4 prev[2];
    if (temporal) {   // in flight beside the source rows
        prev[0] = sse_load16(sto, pt, p.w, vt, x, row[0], n, p.h);
        prev[1] = sse_load16(sto, pt, p.w, vt, x, row[1], n, p.h);
    }
    unsigned se[2][4], so[2][4];   // the stage-1 result as pairs
    if (Ss == 0) {
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const unsigned w[4] = {r[pass].x, r[pass].y, r[pass].z, r[pass].w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                se[pass][k] = w[k] & 0x00ff00ffu;
                so[pass][k] = (w[k] >> 8) & 0x00ff00ffu;
            }
        }
    } else {
        const bool first = m == 0, last = m == kStripMB - 1;
        const int hy = i == 0 ? sp.y0 - 1 : sp.y0 + 16;
        const int hrow = ((i != 0 && i != 7) || hy < 0) ? p.h : hy;   // a row above the picture reads as one below it: nothing; lanes 1 .. 6 have no halo row
        const int rows[3] = {row[0], row[1], hrow};
        uint4 v[3];
        unsigned el[3], er[3], lr[3];
#pragma unroll
        for (int pass = 0; pass < 3; pass++) {   // every load in flight before the first exchange
            v[pass] = pass < 2 ? r[pass] : sse_load16(src, ps, ss, vs, x, rows[pass], n, p.h);
            el[pass] = (first && x > 0) ? ssim_load4(src, ps, ss, vs, x - 4, rows[pass], 4, p.h) : 0u;
            er[pass] = last ? ssim_load4(src, ps, ss, vs, x + 16, rows[pass], left - 16, p.h) : 0u;
        }
#pragma unroll
        for (int pass = 0; pass < 3; pass++) {   // column x - 1 into byte 0 and column x + 16 into byte 1 of one dword
            const unsigned nl = (unsigned)__shfl((int)v[pass].w, (lane - 8) & 63), nr = (unsigned)__shfl((int)v[pass].x, (lane + 8) & 63);
            lr[pass] = ((first ? el[pass] : nl) >> 24) | (((last ? er[pass] : nr) & 0xffu) << 8);
        }
        // which pairs lie outside the picture: column x - 1 exists from the second segment on, column x + j (j up to 16) while j < left
        DnRow mark;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned c0 = 4 * k < left ? 0u : kDnOutside, c1 = 4 * k + 1 < left ? 0u : kDnOutside, c2 = 4 * k + 2 < left ? 0u : kDnOutside,
                           c3 = 4 * k + 3 < left ? 0u : kDnOutside, c4 = 4 * k + 4 < left ? 0u : kDnOutside;
            const unsigned cm = k == 0 ? (x > 0 ? 0u : kDnOutside) : (4 * k - 1 < left ? 0u : kDnOutside);
            mark.e[k] = c0 | (c2 << 16);
            mark.o[k] = c1 | (c3 << 16);
            mark.l[k] = cm | (c1 << 16);
            mark.r[k] = c2 | (c4 << 16);
        }
        const int base = lane & ~7, pl = base | ((i - 1) & 7), nx = base | ((i + 1) & 7);
        uint4 pA, nA, pB, nB;
        unsigned pAl, nAl, pBl, nBl;
        dn_ring(v[0], lr[0], pl, nx, pA, pAl, nA, nAl);
        dn_ring(v[1], lr[1], pl, nx, pB, pBl, nB, nBl);
        const pk16 s2 = pk_splat(2 * Ss), ns2 = pk_splat(-2 * Ss);
        const unsigned all_out = kDnOutside | (kDnOutside << 16);
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            // row above / below: the halo for lane 0's first and lane 7's second row, lane 7's first row above lane 0's second, lane 0's second below lane 7's first
            const uint4 &uv = pass == 0 ? (i == 0 ? v[2] : pA) : (i == 0 ? pA : pB);
            const unsigned ulr = pass == 0 ? (i == 0 ? lr[2] : pAl) : (i == 0 ? pAl : pBl);
            const uint4 &dv = pass == 0 ? (i == 7 ? nB : nA) : (i == 7 ? v[2] : nB);
            const unsigned dlr = pass == 0 ? (i == 7 ? nBl : nAl) : (i == 7 ? lr[2] : nBl);
            const int y = row[pass];
            DnRow U, C, D;
            dn_unpack(U, uv, ulr << 24, ulr >> 8, mark, (y - 1 < 0 || y - 1 >= p.h) ? all_out : 0u);
            dn_unpack(C, v[pass], lr[pass] << 24, lr[pass] >> 8, mark, 0u);
            dn_unpack(D, dv, dlr << 24, dlr >> 8, mark, y + 1 >= p.h ? all_out : 0u);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                se[pass][k] = pk_bits(dn_spatial(pk_of(C.e[k] & 0x00ff00ffu), U.l[k], U.e[k], U.o[k], C.l[k], C.o[k], D.l[k], D.e[k], D.o[k], s2, ns2));
                so[pass][k] = pk_bits(dn_spatial(pk_of(C.o[k] & 0x00ff00ffu), U.e[k], U.o[k], U.r[k], C.e[k], C.r[k], D.e[k], D.o[k], D.r[k], s2, ns2));
            }
        }
    }
    if (temporal) {
        const pk16 t2 = pk_splat(2 * St), nt2 = pk_splat(-2 * St);
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const unsigned w[4] = {prev[pass].x, prev[pass].y, prev[pass].z, prev[pass].w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                se[pass][k] = pk_bits(dn_temporal(pk_of(se[pass][k]), pk_of(w[k] & 0x00ff00ffu), t2, nt2));
                so[pass][k] = pk_bits(dn_temporal(pk_of(so[pass][k]), pk_of((w[k] >> 8) & 0x00ff00ffu), t2, nt2));
            }
        }
    }
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int y = row[pass];
        if (y >= p.h || n <= 0) continue;
        // a sample outside the picture may hold anything in its 16 bits: only the low byte of each half goes back
        const unsigned wds[4] = {(se[pass][0] & 0x00ff00ffu) | ((so[pass][0] & 0x00ff00ffu) << 8), (se[pass][1] & 0x00ff00ffu) | ((so[pass][1] & 0x00ff00ffu) << 8),
                                 (se[pass][2] & 0x00ff00ffu) | ((so[pass][2] & 0x00ff00ffu) << 8), (se[pass][3] & 0x00ff00ffu) | ((so[pass][3] & 0x00ff00ffu) << 8)};
        uint8_t *outs[2] = {pd + (long)y * p.w + x, pt + (long)y * p.w + x};
        const bool vec[2] = {vd, vt};
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t == 1 && !commit) continue;
            if (vec[t] && n == 16) {
                *reinterpret_cast<uint4 *>(outs[t]) = make_uint4(wds[0], wds[1], wds[2], wds[3]);
            } else {
#pragma unroll
                for (int b = 0; b < 16; b++)
                    if (b < n) outs[t][b] = (uint8_t)(wds[b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

}  // namespace pfv
