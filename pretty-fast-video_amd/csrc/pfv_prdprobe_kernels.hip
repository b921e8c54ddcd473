// pfv_prdprobe_kernels.hip -- the p-frame rate-distortion probe (gfx950): payload size AND squared error of a frame as a p-frame against the
// session's prev_frame at EVERY rung of the quality ladder, from one motion search and one forward transform of the residual.
//
// Residuals are halved (src/common.rs:118-119, :304), so a p-frame is often the smaller frame and the worse-looking one, and a macroblock
// that is skipped costs nothing and keeps whatever error its patch has.  The size probe (pfv_pprobe_kernels.hip) holds what does not depend on
// the rung in registers -- source rows, patch rows, the scaled residual coefficients nn; what a rung adds for distortion is the closed loop's
// second half where the macroblock is coded and nothing where it is not.
//
//   k_probe_pframe_rd  k_probe_pframe's front end (tile mapping, issue_window, penc_search<true>, the residual's forward transform up to nn),
//                      then probe_rung_loop exactly as the size probe calls it (the same accumulator rows: sizes and the 20 counts are the
//                      size probe's), then the distortion loop:
//                        skipped at rung r ((float)err <= min_err[r])  the reconstruction is the patch: sum (src - patch)^2 over the pixels
//                                          inside the picture, formed ONCE (SearchOut::err covers the padded 16 x 16 block and cannot stand in);
//                        coded at rung r   rd_recon_row<FLT, true>: q = trunc(n * rcp), the INTER dequantiser products of rung r (indexed by
//                                          zigzag position, as decode does), inverse columns, transpose, inverse rows, apply_residuals
//                                          (patch + 2 * min(t, 127), saturated) -- penc_half's second half with the rung's constants.
//                      The transposes need every lane, so a rung reconstructs all 8 macroblocks of the wavefront and each takes its own answer;
//                      a rung at which NO macroblock of the wavefront is coded (a wavefront-uniform test) runs no inverse at all.  Squared
//                      error as rd_rung_loop forms it: v_dot4_u32_u8, rd_picture_mask on both operands, mb_sum, ONE 64-bit vector atomic per
//                      wavefront and rung into sse_acc[stream][rung][plane].  A tile lies in one plane: the inter reciprocals, dequantiser
//                      products and min_err of all rungs are staged once per workgroup for that plane.
//   k_pprobe_rd_sizes  k_pprobe_sizes's row body and, in the same wavefront, the three plane sums of its (stream, rung) moved out and
//                      cleared (k_probe_rd_sizes's tail): no host-side clear, no synchronisation, replays from a graph.  A plain kernel,
//                      not a template instance: linkonce bodies shifted the benched kernels' code (profiles/pframe_probe.md).
// 8 lanes per macroblock only, as k_probe_pframe.  Included by pfv_capi.hip behind pfv_pprobe_kernels.hip.
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
    uint8_t *win = win_lds + 16;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = lane >> 3, i = lane & 7;
    const int vt = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const TilePos cur = locate_tile(g, vt, wave);
    const PlaneGeom &p = g.p[cur.sp.plane];
    // as k_probe_pframe, and the inter dequantiser products (decode's index) next to the reciprocals
    if (wave == 0) {
        fill_qtable<true, FLT>(qtab_lds, qtabs + 2 + p.qsel, lane);
        if (lane < n_rungs) err_lds[lane] = min_err[lane];
    }
    for (int r = wave; r < n_rungs; r += kStripsPerWG) {
        const QTab *qt = qtabs + 4 * r + 2 + p.qsel;
        rcp_lds[r][lane] = qt->rcp[lane];
        deq_lds[r][lane] = FLT ? __float_as_int((float)qt->deq[lane]) : qt->deq[lane];   // float form: deq < 2^24 (checked on the host)
    }
    issue_window(p, ref + (long)cur.sp.stream * g.pad_frame_bytes + p.pad_off, cur, win, wave, lane);
    uint4 rows[2];
    rows[0] = rows[1] = make_uint4(0, 0, 0, 0);
    if (cur.wave_valid) {
        const uint8_t *plane = frame_src(g, src, cur.sp.stream) + p.src_off;
        rows[0] = load_src16(plane, p, cur.sp.x0 + m * 16, cur.sp.y0 + i);
        rows[1] = load_src16(plane, p, cur.sp.x0 + m * 16, cur.sp.y0 + i + 8);
    }
    __syncthreads();   // window complete (vmcnt drained at the barrier); the tables are visible
    SearchOut so;
    so.cx = so.cy = so.err = 0; so.coded = false;
    so.patch[0] = so.patch[1] = make_uint4(0, 0, 0, 0);
    if (cur.wave_valid) penc_search<true>(g, cur, win, red_lds, rows, lane, 0.0f, neg2, so);   // the skip test is taken per rung below
    __syncthreads();   // window released by every wavefront: its slices become the exchange regions
    if (!cur.wave_valid) return;   // no barrier behind this point

    int *xw = reinterpret_cast<int *>(win + win_first_issue(wave) * 1024);
    int *mb = xw + m * kMBPitch;
    const LaneQ lq{qtab_lds, i};
    // n = (m * SCALE) >> 16 of the residual, column layout, as k_probe_pframe
    f2 nn[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (FLT) {
            f2 x[8], pp[8];
            unpack_row_f(rows[h], x);
            unpack_row_f(so.patch[h], pp);
#pragma unroll
            for (int k = 0; k < 8; k++) x[k] = residual_f(x[k], pp[k]);   // calc_residuals (:118-119), delta / 2 truncating, << 8 (:304)
            ffdct8(x);
            f_rows_to_cols(x, mb, i, m & 3);
            ffdct8(x);
#pragma unroll
            for (int k = 0; k < 8; k++) nn[h][k] = quant_scale(x[k], lq.scale(k));
        } else {   // penc_half's integer arithmetic
            int v[2][8], pp[2][8];
            unpack_row(rows[h], v);
            unpack_row(so.patch[h], pp);
#pragma unroll
            for (int s = 0; s < 2; s++) {
#pragma unroll
                for (int k = 0; k < 8; k++) v[s][k] = (int)((unsigned)tdiv2(v[s][k] - pp[s][k]) << 8);
            }
            fdct8(v[0]);
            fdct8(v[1]);
            rows_to_cols2(v, mb, i, m & 3);
            fdct8(v[0]);
            fdct8(v[1]);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int scale = lq.scale(k);
                nn[h][k] = f2{(float)(wmul24(v[0][k], scale) >> 16), (float)(wmul24(v[1][k], scale) >> 16)};
            }
        }
    }
    const bool mb_valid = m < cur.sp.n_mb;   // macroblocks beyond the strip's end count nothing (and lie outside the picture: their mask is empty)
    const float err = (float)so.err;

    // distortion.  a = the source rows, b = the reconstruction, both with the pixels outside the picture zeroed:
    // sum (a - b)^2 = sum a^2 - 2 sum ab + sum b^2 per lane, exact in u32 (a lane: < 32 x 255^2)
    // This loop runs BEFORE the size loop although it reads nothing of it and writes other accumulators: the source and patch rows end here,
    // and kept alive across probe_rung_loop they cost the second wavefront per SIMD (281 registers against 256).  The masks are formed here,
    // behind the search, for the same reason.
    uint4 mask[2];
    uint32_t aa = 0, skip_ab = 0, skip_bb = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        mask[h] = rd_picture_mask(p, cur.sp.x0 + m * 16, cur.sp.y0 + i + 8 * h);
        rows[h] = make_uint4(rows[h].x & mask[h].x, rows[h].y & mask[h].y, rows[h].z & mask[h].z, rows[h].w & mask[h].w);
        const uint4 b = make_uint4(so.patch[h].x & mask[h].x, so.patch[h].y & mask[h].y, so.patch[h].z & mask[h].z, so.patch[h].w & mask[h].w);
        aa = sq4(rows[h].x, rows[h].y, rows[h].z, rows[h].w, aa);
        skip_ab = dot_ab(rows[h], b.x, b.y, b.z, b.w, skip_ab);
        skip_bb = sq4(b.x, b.y, b.z, b.w, skip_bb);
    }
    const uint32_t skip_sse = aa + skip_bb - 2u * skip_ab;   // the lane's share when its macroblock is skipped: the same at every rung
    unsigned long long *sums = sse_acc + ((size_t)cur.sp.stream * n_rungs) * 3 + cur.sp.plane;
    for (int r = 0; r < n_rungs; r++) {
        const bool coded = mb_valid && !(err <= err_lds[r]);
        uint32_t lane_sse = skip_sse;
        if (__ballot(coded) != 0ull) {   // wavefront-uniform: the transposes below need all 64 lanes
            uint32_t ab = 0, bb = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                uint4 b = rd_recon_row<FLT, true>(nn[h], &rcp_lds[r][0], &deq_lds[r][0], xw, m, i, so.patch[h]);
                b = make_uint4(b.x & mask[h].x, b.y & mask[h].y, b.z & mask[h].z, b.w & mask[h].w);
                ab = dot_ab(rows[h], b.x, b.y, b.z, b.w, ab);
                bb = sq4(b.x, b.y, b.z, b.w, bb);
            }
            if (coded) lane_sse = aa + bb - 2u * ab;
        }
        const int mine = mb_sum((int)lane_sse);   // a macroblock: < 2^24; the wavefront: < 2^27
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) total += (uint32_t)__builtin_amdgcn_readlane(mine, 8 * j);
        if (lane == 0 && total) atomicAdd(&sums[(size_t)r * 3], (unsigned long long)total);
    }

    // sizes and counts: the size probe's own loops over the same registers
    int zz[8];
#pragma unroll
    for (int k = 0; k < 8; k++) zz[k] = lq.zz(k);
    uint32_t *rows_acc = acc + (size_t)cur.sp.stream * n_rungs * kPProbeAcc;
    probe_rung_loop<8, kPProbeAcc, kPProbeStats>(nn, zz, &rcp_lds[0][0], n_rungs, lane, rows_acc,
                                                 [&](int r) { return mb_valid && !(err <= err_lds[r]); });   // the skip decision (:209, :221) at rung r

    // header bits and the coded count per rung, as k_probe_pframe
    const bool first = mb_valid && i == 0, moved = first && (so.cx != 0 || so.cy != 0);
    const uint32_t n_moved = (uint32_t)__builtin_popcountll(__ballot(moved));
    const uint32_t hdr_bits = 2u * (uint32_t)__builtin_popcountll(__ballot(first)) + 14u * n_moved;
    for (int r = 0; r < n_rungs; r++) {
        const uint32_t n_coded = (uint32_t)__builtin_popcountll(__ballot(first && !(err <= err_lds[r])));
        const uint32_t mine = lane == kPProbeCodedAt ? n_coded : (lane == kPProbeMovedAt ? n_moved : hdr_bits);
        if (lane >= kPProbeCodedAt && lane <= kPProbeHdrAt && mine) atomicAdd(&rows_acc[(size_t)r * kPProbeAcc + lane], mine);
    }
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
    const size_t at = (size_t)blockIdx.x * 3 + threadIdx.x;
    if (threadIdx.x < 3) {
        sse[at] = sse_acc[at];
        sse_acc[at] = 0;   // consumed: the next call starts clean
    }
}

}  // namespace pfv
