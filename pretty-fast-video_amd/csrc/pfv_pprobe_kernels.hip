// pfv_pprobe_kernels.hip -- the p-frame size probe (gfx950): the payload size of a frame as a p-frame against the session's prev_frame at EVERY
// rung of the quality ladder, from one motion search and one forward transform of the residual.
//
// The 4-step search (src/common.rs:154-204) reads only the source and prev_frame, so its vector, its patch and its best error are the same at
// every rung.  Two things depend on the rung: the skip test best_err <= px_err^2 * 256 (:209, :221) and the quantiser's trunc(n * rcp).  A
// payload's size is the closed function of pfv_probe_kernels.hip plus the block headers: 2 bits per macroblock, 16 where the vector is not zero
// (k_ent_scan), whether or not the macroblock is coded.
//
//   k_probe_pframe  decomposition of k_pf_search: one workgroup per 128 x 64 tile, the reference window staged by issue_window, source rows in
//                   registers, penc_search (register reduce-scatter: no reduction regions) -> vector, patch rows, best error.  Behind the
//                   window-release barrier each wavefront transforms its own 8 macroblocks in its slice of the window: per half macroblock
//                   the residual as penc_half forms it, rows, transpose, columns, quant_scale -- the scaled coefficients stay in registers
//                   as in k_probe_iframe; no coefficient, header or reconstruction is stored, no inverse transform runs.  Then
//                   probe_rung_loop with the inter reciprocals and min_err of all rungs staged in LDS once: at rung r a macroblock counts
//                   when it exists and !((float)err <= min_err[r]).  Three more words per (stream, rung) row: coded macroblocks, macroblocks
//                   with a non-zero vector and header bits -- one vector atomic per wavefront for the three.
//   k_pprobe_sizes (pfv_probe_kernels.hip, k_probe_sizes' sibling over one body) turns the rows into sizes and clears them.
// 8 lanes per macroblock only: PFV_OPT_LANE_MAPPING does not apply (a probe of few streams is a small launch either way).
// Included by pfv_capi.hip behind pfv_probe_kernels.hip: the main translation unit, default scheduling.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfv {

template <bool FLT>
__global__ __launch_bounds__(kThreads) void k_probe_pframe(FrameGeom g, const uint8_t *__restrict__ src, const uint8_t *__restrict__ ref,
                                                            const QTab *__restrict__ qtabs, int n_rungs, const float *__restrict__ min_err, int neg2,
                                                            uint32_t *__restrict__ acc)
{
    __shared__ __attribute__((aligned(16))) uint8_t win_lds[16 + kWinAlloc];
    __shared__ __attribute__((aligned(16))) int red_lds[4];                    // penc_search<true> takes the pointer and never uses it
    __shared__ __attribute__((aligned(16))) int qtab_lds[kQTabDwords];
    __shared__ float rcp_lds[kProbeMaxRungs][64];
    __shared__ float err_lds[kProbeMaxRungs];
    uint8_t *win = win_lds + 16;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = lane >> 3, i = lane & 7;
    const int vt = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const TilePos cur = locate_tile(g, vt, wave);
    const PlaneGeom &p = g.p[cur.sp.plane];
    // a tile lies in one plane: one copy per workgroup.  Scale and zigzag position do not depend on the rung (the entry's reciprocal is rung
    // 0's and is not used); the inter reciprocals (inter_l / inter_c) of all rungs, a rung per wavefront in turn
    if (wave == 0) {
        fill_qtable<true, FLT>(qtab_lds, qtabs + 2 + p.qsel, lane);
        if (lane < n_rungs) err_lds[lane] = min_err[lane];
    }
    for (int r = wave; r < n_rungs; r += kStripsPerWG) rcp_lds[r][lane] = qtabs[4 * r + 2 + p.qsel].rcp[lane];
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
    // n = (m * SCALE) >> 16 of the residual, column layout: nn[h][k] = rows k of subblocks 2h and 2h + 1, column i
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
    int zz[8];
#pragma unroll
    for (int k = 0; k < 8; k++) zz[k] = lq.zz(k);
    const bool mb_valid = m < cur.sp.n_mb;   // macroblocks beyond the strip's end count nothing
    const float err = (float)so.err;
    uint32_t *rows_acc = acc + (size_t)cur.sp.stream * n_rungs * kPProbeAcc;
    probe_rung_loop<8, kPProbeAcc, kPProbeStats>(nn, zz, &rcp_lds[0][0], n_rungs, lane, rows_acc,
                                                 [&](int r) { return mb_valid && !(err <= err_lds[r]); });   // the skip decision (:209, :221) at rung r

    // per macroblock, whatever the rung: the header's 2 bits (has_mv, has_coeff) and 14 more where the vector is not zero; per rung: coded or not
    const bool first = mb_valid && i == 0, moved = first && (so.cx != 0 || so.cy != 0);
    const uint32_t n_moved = (uint32_t)__builtin_popcountll(__ballot(moved));
    const uint32_t hdr_bits = 2u * (uint32_t)__builtin_popcountll(__ballot(first)) + 14u * n_moved;
    for (int r = 0; r < n_rungs; r++) {
        const uint32_t n_coded = (uint32_t)__builtin_popcountll(__ballot(first && !(err <= err_lds[r])));
        const uint32_t mine = lane == kPProbeCodedAt ? n_coded : (lane == kPProbeMovedAt ? n_moved : hdr_bits);
        if (lane >= kPProbeCodedAt && lane <= kPProbeHdrAt && mine) atomicAdd(&rows_acc[(size_t)r * kPProbeAcc + lane], mine);
    }
}

}  // namespace pfv
