// pfv_prdprobe_kernels.hip -- the p-frame rate-distortion probe (gfx950): payload size AND squared error of a frame as a p-frame against the
// session's prev_frame at EVERY rung of the quality ladder, from one motion search and one forward transform of the residual.
//
// Residuals are halved (src/common.rs:118-119, :304), so a p-frame is often the smaller frame and the worse-looking one, and a macroblock
// that is skipped costs nothing and keeps whatever error its patch has.  The size probe (pfv_pprobe_kernels.hip) holds what does not depend on
// the rung in registers -- source rows, patch rows, the scaled residual coefficients nn; what a rung adds for distortion is the closed loop's
// second half where the macroblock is coded and nothing where it is not.
//
//   k_probe_pframe_rd  probe_tile_front<FLT, true> and probe_forward_row<FLT, true> (the size probe's front end with the inter dequantiser
//                      products staged next to the reciprocals), then the distortion loop, then probe_rung_loop and pprobe_header_tail
//                      exactly as the size probe calls them (the same accumulator rows: sizes and the 20 counts are the size probe's).
//                      One predicate object, coded_at, serves all three.  The distortion loop:
//                        skipped at rung r ((float)err <= min_err[r])  the reconstruction is the patch: sum (src - patch)^2 over the pixels
//                                          inside the picture, formed ONCE (SearchOut::err covers the padded 16 x 16 block and cannot stand in);
//                        coded at rung r   rd_recon_row<FLT, true>: q = trunc(n * rcp), the INTER dequantiser products of rung r (indexed by
//                                          zigzag position, as decode does), inverse columns, transpose, inverse rows, apply_residuals
//                                          (patch + 2 * min(t, 127), saturated) -- penc_half's second half with the rung's constants.
//                      The transposes need every lane, so a rung reconstructs all 8 macroblocks of the wavefront and each takes its own answer;
//                      a rung at which NO macroblock of the wavefront is coded (a wavefront-uniform test) runs no inverse at all.  Squared
//                      error as rd_rung_loop forms it: v_dot4_u32_u8, rd_picture_mask on both operands, rd_sse_out (mb_sum, ONE 64-bit vector
//                      atomic per wavefront and rung into sse_acc[stream][rung][plane]).  A tile lies in one plane: the inter reciprocals, dequantiser
//                      products and min_err of all rungs are staged once per workgroup for that plane.
//   k_pprobe_rd_sizes  k_pprobe_sizes's row body and, in the same wavefront, the three plane sums of its (stream, rung) moved out and
//                      cleared (rd_sums_out): no host-side clear, no synchronisation, replays from a graph.  A plain kernel,
//                      not a template instance: linkonce bodies shifted the benched kernels' code (profiles/pframe_probe.md).
// 8 lanes per macroblock only.  Included by pfv_capi.hip behind pfv_pprobe_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfv {

template <bool FLT>
__global__ __launch_bounds__(kThreads) void k_probe_pframe_rd(FrameGeom g, const uint8_t *__restrict__ src, const uint8_t *__restrict__ ref,
                                                               const QTab *__restrict__ qtabs, int n_rungs, const float *__restrict__ min_err, int neg2,
                                                               uint32_t *__restrict__ acc, unsigned long long *__restrict__ sse_acc)
{
    __shared__ __attribute__((aligned(16))) uint8_t win_lds[16 + kWinAlloc];
    __shared__ __attribute__((aligned(16))) int red_lds[4];                    // penc_search<true> takes the pointer and never uses it
    __shared__ __attribute__((aligned(16))) int qtab_lds[kQTabDwords];
    __shared__ float rcp_lds[kProbeMaxRungs][64];
    __shared__ int deq_lds[kProbeMaxRungs][64];
    __shared__ float err_lds[kProbeMaxRungs];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = lane >> 3, i = lane & 7;
    uint4 rows[2];
    SearchOut so;
    int *xw;
    const TilePos cur = probe_tile_front<FLT, true>(g, src, ref, qtabs, n_rungs, min_err, neg2, win_lds + 16, red_lds, qtab_lds, rcp_lds, deq_lds, err_lds, lane, wave, rows, so, xw);
    if (!cur.wave_valid) return;   // no barrier behind this point

    const PlaneGeom &p = g.p[cur.sp.plane];
    const LaneQ lq{qtab_lds, i};
    f2 nn[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++) probe_forward_row<FLT, true>(rows[h], so.patch[h], xw + m * kMBPitch, i, m & 3, lq, nn[h]);
    const bool mb_valid = m < cur.sp.n_mb;   // macroblocks beyond the strip's end count nothing (and lie outside the picture: their mask is empty)
    const float err = (float)so.err;
    const auto coded_at = [&](int r) { return mb_valid && !(err <= err_lds[r]); };   // the skip decision (:209, :221) at rung r

    // distortion, in front of the size loop.  a = the source rows, b = the reconstruction, both with the pixels outside the picture zeroed:
    // sum (a - b)^2 = sum a^2 - 2 sum ab + sum b^2 per lane, exact in u32 (a lane: < 32 x 255^2)
    uint4 mask[2];
    uint32_t aa = 0, skip_ab = 0, skip_bb = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        mask[h] = rd_picture_mask(p, cur.sp.x0 + m * 16, cur.sp.y0 + i + 8 * h);
        rows[h] = and4(rows[h], mask[h]);
        const uint4 b = and4(so.patch[h], mask[h]);
        aa = sq4(rows[h].x, rows[h].y, rows[h].z, rows[h].w, aa);
        skip_ab = dot_ab(rows[h], b.x, b.y, b.z, b.w, skip_ab);
        skip_bb = sq4(b.x, b.y, b.z, b.w, skip_bb);
    }
    const uint32_t skip_sse = aa + skip_bb - 2u * skip_ab;   // the lane's share when its macroblock is skipped: the same at every rung
    unsigned long long *sums = sse_acc + ((size_t)cur.sp.stream * n_rungs) * 3 + cur.sp.plane;
    for (int r = 0; r < n_rungs; r++) {
        const bool coded = coded_at(r);
        uint32_t lane_sse = skip_sse;
        if (__ballot(coded) != 0ull) {   // wavefront-uniform: the transposes below need all 64 lanes
            uint32_t ab = 0, bb = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint4 b = and4(rd_recon_row<FLT, true>(nn[h], &rcp_lds[r][0], &deq_lds[r][0], xw, m, i, so.patch[h]), mask[h]);
                ab = dot_ab(rows[h], b.x, b.y, b.z, b.w, ab);
                bb = sq4(b.x, b.y, b.z, b.w, bb);
            }
            if (coded) lane_sse = aa + bb - 2u * ab;
        }
        rd_sse_out(lane_sse, lane, &sums[(size_t)r * 3]);
    }

    // sizes and counts: the size probe's own loops over the same registers
    int zz[8];
#pragma unroll
    for (int k = 0; k < 8; k++) zz[k] = lq.zz(k);
    uint32_t *rows_acc = acc + (size_t)cur.sp.stream * n_rungs * kPProbeAcc;
    probe_rung_loop<8, kPProbeAcc, kPProbeStats>(nn, zz, &rcp_lds[0][0], n_rungs, lane, rows_acc, coded_at);
    pprobe_header_tail(mb_valid, so, n_rungs, lane, rows_acc, coded_at);
}

// One wavefront per (stream, rung): k_pprobe_sizes's row, then the plane sums of the same (stream, rung) out and cleared
__global__ __launch_bounds__(64) void k_pprobe_rd_sizes(uint32_t *__restrict__ acc, uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats,
                                                        unsigned long long *__restrict__ sse_acc, unsigned long long *__restrict__ sse)
{
    __shared__ int32_t hist[16];
    __shared__ uint32_t val[16];
    __shared__ uint8_t len[16], table[16];
    __shared__ int parent[32], branch[32];
    probe_sizes_row<true>(acc, sizes, stats, hist, table, val, len, parent, branch);
    rd_sums_out(sse_acc, sse);
}

}  // namespace pfv
