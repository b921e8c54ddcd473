// pfv_pprobe_kernels.hip -- the p-frame size probe (gfx950): the payload size of a frame as a p-frame against the session's prev_frame at EVERY
// rung of the quality ladder, from one motion search and one forward transform of the residual.
//
// The 4-step search (src/common.rs:154-204) reads only the source and prev_frame, so its vector, its patch and its best error are the same at
// every rung.  Two things depend on the rung: the skip test best_err <= px_err^2 * 256 (:209, :221) and the quantiser's trunc(n * rcp).  A
// payload's size is the closed function of pfv_probe_kernels.hip plus the block headers: 2 bits per macroblock, 16 where the vector is not zero
// (k_ent_scan), whether or not the macroblock is coded.
//
//   probe_tile_front    the tile probes' front end (k_probe_pframe, _rd, _ssim), the decomposition of k_pf_search: one workgroup per 128 x 64
//                       tile, tables and min_err of all rungs staged in LDS once, the reference window staged by issue_window, source rows in
//                       registers, penc_search (register reduce-scatter: no reduction regions) -> vector, patch rows, best error.
//   k_probe_pframe      behind the window-release barrier each wavefront transforms its own 8 macroblocks in its slice of the window:
//                       probe_forward_row<FLT, true> per half macroblock -- the scaled coefficients stay in registers as in k_probe_iframe; no
//                       coefficient, header or reconstruction is stored, no inverse transform runs.  Then probe_rung_loop with the inter
//                       reciprocals: at rung r a macroblock counts when it exists and !((float)err <= min_err[r]) -- ONE predicate object per
//                       kernel, handed to every loop that asks.
//   pprobe_header_tail  three more words per (stream, rung) row: coded macroblocks, macroblocks with a non-zero vector and header bits -- one
//                       vector atomic per wavefront for the three.
//   k_pprobe_sizes (pfv_probe_kernels.hip, k_probe_sizes' sibling over one body) turns the rows into sizes and clears them.
// 8 lanes per macroblock only: PFV_OPT_LANE_MAPPING does not apply (a probe of few streams is a small launch either way).
// Included by pfv_capi.hip behind pfv_probe_kernels.hip: the main translation unit, default scheduling.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfv {

// The tile probes' front end, through the window-release barrier.  The LDS arrays are the kernel's: win = its window, qtab / rcp / err (and deq
// where DEQ: the inter dequantiser products, decode's index, f32 bits in the float form -- deq < 2^24, checked on the host) are filled here.
// A tile lies in one plane: one copy per workgroup.  Scale and zigzag position do not depend on the rung (the entry's reciprocal is rung 0's
// and is not used); the inter tables (inter_l / inter_c) of all rungs, a rung per wavefront in turn.  -> rows = the lane's source rows, so =
// the search's answer (the skip test is the kernel's, per rung), xw = the wavefront's exchange region, a slice of the released window.
// The kernel returns behind this call where !wave_valid: no barrier from there on.  The picture masks are NOT formed here: they are formed
// behind the search, next to their use (the register argument at probe_strip_front).
template <bool FLT, bool DEQ>
__device__ __forceinline__ TilePos probe_tile_front(const FrameGeom &g, const uint8_t *src, const uint8_t *ref, const QTab *qtabs,
                                                    int n_rungs, const float *min_err, int neg2, uint8_t *win, int *red, int *qtab,
                                                    float (*rcp)[64], int (*deq)[64], float *err, int lane, int wave, uint4 (&rows)[2], SearchOut &so, int *&xw)
{
    const int m = lane >> 3, i = lane & 7;
    const int vt = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const TilePos cur = locate_tile(g, vt, wave);
    const PlaneGeom &p = g.p[cur.sp.plane];
    if (wave == 0) {
        fill_qtable<true, FLT>(qtab, qtabs + 2 + p.qsel, lane);
        if (lane < n_rungs) err[lane] = min_err[lane];
    }
    for (int r = wave; r < n_rungs; r += kStripsPerWG) {
        const QTab *qt = qtabs + 4 * r + 2 + p.qsel;
        rcp[r][lane] = qt->rcp[lane];
        if (DEQ) deq[r][lane] = FLT ? __float_as_int((float)qt->deq[lane]) : qt->deq[lane];
    }
    issue_window(p, ref + (long)cur.sp.stream * g.pad_frame_bytes + p.pad_off, cur, win, wave, lane);
    rows[0] = rows[1] = make_uint4(0, 0, 0, 0);
    if (cur.wave_valid) {
        const uint8_t *plane = frame_src(g, src, cur.sp.stream) + p.src_off;
        rows[0] = load_src16(plane, p, cur.sp.x0 + m * 16, cur.sp.y0 + i);
        rows[1] = load_src16(plane, p, cur.sp.x0 + m * 16, cur.sp.y0 + i + 8);
    }
    __syncthreads();   // window complete (vmcnt drained at the barrier); the tables are visible
    so.cx = so.cy = so.err = 0; so.coded = false;
    so.patch[0] = so.patch[1] = make_uint4(0, 0, 0, 0);
    if (cur.wave_valid) penc_search<true>(g, cur, win, red, rows, lane, 0.0f, neg2, so);
    __syncthreads();   // window released by every wavefront: its slices become the exchange regions
    xw = reinterpret_cast<int *>(win + win_first_issue(wave) * 1024);
    return cur;
}

// Per macroblock, whatever the rung: the header's 2 bits (has_mv, has_coeff) and 14 more where the vector is not zero; per rung: coded or not
// (coded_at(r): the kernel's skip predicate).  The kPProbeCodedAt..kPProbeHdrAt words of the wavefront's rows.
template <class Coded>
__device__ __forceinline__ void pprobe_header_tail(bool mb_valid, const SearchOut &so, int n_rungs, int lane, uint32_t *rows_acc, Coded &&coded_at)
{
    const bool first = mb_valid && (lane & 7) == 0, moved = first && (so.cx != 0 || so.cy != 0);
    const uint32_t n_moved = (uint32_t)__builtin_popcountll(__ballot(moved));
    const uint32_t hdr_bits = 2u * (uint32_t)__builtin_popcountll(__ballot(first)) + 14u * n_moved;
    for (int r = 0; r < n_rungs; r++) {
        const uint32_t n_coded = (uint32_t)__builtin_popcountll(__ballot(first && coded_at(r)));
        const uint32_t mine = lane == kPProbeCodedAt ? n_coded : (lane == kPProbeMovedAt ? n_moved : hdr_bits);
        if (lane >= kPProbeCodedAt && lane <= kPProbeHdrAt && mine) atomicAdd(&rows_acc[(size_t)r * kPProbeAcc + lane], mine);
    }
}

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

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = lane >> 3, i = lane & 7;
    uint4 rows[2];
    SearchOut so;
    int *xw;
    const TilePos cur = probe_tile_front<FLT, false>(g, src, ref, qtabs, n_rungs, min_err, neg2, win_lds + 16, red_lds, qtab_lds, rcp_lds, nullptr, err_lds, lane, wave, rows, so, xw);
    if (!cur.wave_valid) return;   // no barrier behind this point

    const LaneQ lq{qtab_lds, i};
    f2 nn[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++) probe_forward_row<FLT, true>(rows[h], so.patch[h], xw + m * kMBPitch, i, m & 3, lq, nn[h]);
    int zz[8];
#pragma unroll
    for (int k = 0; k < 8; k++) zz[k] = lq.zz(k);
    const bool mb_valid = m < cur.sp.n_mb;   // macroblocks beyond the strip's end count nothing
    const float err = (float)so.err;
    const auto coded_at = [&](int r) { return mb_valid && !(err <= err_lds[r]); };   // the skip decision (:209, :221) at rung r
    uint32_t *rows_acc = acc + (size_t)cur.sp.stream * n_rungs * kPProbeAcc;
    probe_rung_loop<8, kPProbeAcc, kPProbeStats>(nn, zz, &rcp_lds[0][0], n_rungs, lane, rows_acc, coded_at);
    pprobe_header_tail(mb_valid, so, n_rungs, lane, rows_acc, coded_at);
}

}  // namespace pfv
