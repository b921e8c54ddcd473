// pfv_rdprobe_kernels.hip -- the i-frame rate-distortion probe (gfx950): payload size AND squared error of a frame as an i-frame at EVERY rung
// of a session's quality ladder, from one read of the frame.
//
// Fidelity is not monotone in the quantiser here: decode indexes SCALE and q by zigzag position, encode by raster position (src/dct.rs:78-82
// against :92-93), so a finer rung can reconstruct worse than a coarser one.  A policy that wants to know has to measure; the size probe
// (pfv_probe_kernels.hip) already holds everything that does not depend on the rung -- the source rows and the scaled coefficients nn -- in
// registers, and what a rung adds for distortion is the closed loop's second half.
//
//   k_probe_iframe_rd  probe_strip_front (pfv_probe_kernels.hip), then two rung loops over the same registers:
//                        probe_rung_loop   sizes and counts, the size probe's own (into the same accumulator rows);
//                        rd_rung_loop      per rung: q = trunc(n * rcp); q * SCALE[z] q[z] with rung r's table (QTab::deq: indexed by zigzag
//                                          position, as decode does); inverse columns, transpose through the wavefront's exchange region,
//                                          inverse rows; the pixel clamp of src/common.rs:321 -- inverse_half_f<true> / inverse_half of
//                                          k_enc_iframe with the rung's constants; then sum (a - b)^2 = sum a^2 - 2 sum ab + sum b^2 against
//                                          the lane's source row with v_dot4_u32_u8, bytes at x >= w or y >= h masked out of both operands
//                                          (what pfv_frames_sse_dev counts).  mb_sum over the macroblock's lanes, a sum over the wavefront
//                                          (a strip lies in one plane of one stream; 64 lanes x 32 pixels x 255^2 < 2^27), rd_sse_out: ONE
//                                          64-bit vector atomic per wavefront and rung into sse_acc[stream][rung][plane].
//   rd_stage_intra_tables  the reciprocals and dequantiser products of all rungs, staged ONCE PER WORKGROUP for both table sets an i-frame
//                      uses (luma, chroma: 2 x 11 x 64 x 2 dwords = 11 KiB, one barrier), instead of once per wavefront for the wavefront's
//                      plane (4 x 11 x 64 x 2 dwords = 22 KiB): 31 KiB of LDS per workgroup instead of 42.
//   k_probe_rd_sizes   k_probe_sizes's row body (sizes, counts, the rows cleared) and, in the same wavefront, rd_sums_out: the three plane
//                      sums of its (stream, rung) moved to the caller's buffer and cleared -- so the pair of launches needs no host-side
//                      clear and no synchronisation, and can be replayed from a graph.
// Included by pfv_capi.hip behind pfv_probe_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfv {

// byte mask of the 16 pixels x .. x + 15 of row y: 0xff where the pixel lies inside the plane's w x h
__device__ __forceinline__ uint4 rd_picture_mask(const PlaneGeom &p, int x, int y)
{
    const int n = y < p.h ? min(max(p.w - x, 0), 16) : 0;
    uint32_t m[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const int k = min(max(n - 4 * d, 0), 4);
        m[d] = k == 4 ? 0xffffffffu : (1u << (8 * k)) - 1u;
    }
    return make_uint4(m[0], m[1], m[2], m[3]);
}

// The closed loop's second half for one half-macroblock at one rung: nn = the lane's scaled coefficients (column layout), rc / dq = the rung's
// reciprocals and dequantiser products [64] (LDS; dq holds f32 bits in the float form) -> the 16 reconstructed pixels of the lane's row.
// RESIDUAL (the p-frame probe, pfv_prdprobe_kernels.hip): nn is a residual's and `pred` the lane's row of the prediction -- the tail is
// penc_half's apply_residuals (src/common.rs:98-104), pred + 2 * min(t, 127), saturated, in place of the pixel clamp.
template <bool FLT, bool RESIDUAL = false>
__device__ __forceinline__ uint4 rd_recon_row(const f2 (&nn)[8], const float *rc, const int *dq, int *xw, int slot, int i, const uint4 &pred = uint4())
{
    int *mb = xw + slot * kMBPitch;
    if (FLT) {   // inverse_half_f<true> behind quant_div
        f2 c[8];
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = f2trunc(nn[k] * f2s(rc[k * 8 + i])) * f2s(__int_as_float(dq[k * 8 + i]));
        fidct8(c);   // dct_inverse_transform_columns
        f_cols_to_rows(c, mb, i, slot & 3);
        fidct8(c);   // dct_inverse_transform_rows
        if (RESIDUAL) {   // inverse_half_f<false>'s v >> 8, then apply_residuals
            f2 pp[8];
            unpack_row_f(pred, pp);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const f2 t = f2floor(c[k] * f2s(1.0f / 256.0f));
                c[k] = pp[k] + f2{__builtin_fminf(t[0], 127.0f), __builtin_fminf(t[1], 127.0f)} * f2s(2.0f);
            }
            return pack_row_f(c);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = iframe_pixel_f(c[k]);
        return pack_row_f(c);
    }
    int v[2][8];   // inverse_half + the clamp of src/common.rs:321
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const f2 q = f2trunc(nn[k] * f2s(rc[k * 8 + i]));
        const int deq = dq[k * 8 + i];
        v[0][k] = wmul24((int)q[0], deq);
        v[1][k] = wmul24((int)q[1], deq);
    }
    idct8(v[0]);
    idct8(v[1]);
    cols_to_rows2(v, mb, i, slot & 3);
    int pp[2][8];
    if (RESIDUAL) unpack_row(pred, pp);
#pragma unroll
    for (int s = 0; s < 2; s++) {
        idct8(v[s]);
#pragma unroll
        for (int k = 0; k < 8; k++)
            v[s][k] = RESIDUAL ? min(max(pp[s][k] + 2 * min(v[s][k] >> 8, 127), 0), 255) : min(max((v[s][k] >> 8) + 128, 0), 255);
    }
    return pack_row(v);
}

__device__ __forceinline__ uint4 and4(const uint4 &x, const uint4 &m) { return make_uint4(x.x & m.x, x.y & m.y, x.z & m.z, x.w & m.w); }

// the wavefront's sum of the lanes' squared errors into the plane sum of one rung: ONE 64-bit vector atomic
__device__ __forceinline__ void rd_sse_out(uint32_t lane_sse, int lane, unsigned long long *sum)
{
    const int mine = mb_sum((int)lane_sse);   // a lane: < 32 x 255^2; a macroblock: < 2^24; the wavefront: < 2^27
    uint32_t total = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) total += (uint32_t)__builtin_amdgcn_readlane(mine, 8 * j);
    if (lane == 0 && total) atomicAdd(sum, (unsigned long long)total);
}

// The distortion half of the rung loop (k_probe_iframe_rd; the p-frame probes have their own, on residuals and with a skip test per rung): a =
// the lane's source rows with the pixels outside the picture zeroed, mask = those pixels' byte masks, rcp / deq = the constants of all rungs
// [n_rungs][64] (LDS), sums = the 64-bit sum of the wavefront's (stream, plane) at rung 0, PITCH words per rung.
template <bool FLT, int LPM, int PITCH>
__device__ __forceinline__ void rd_rung_loop(const f2 (&nn)[LPM == 8 ? 2 : 1][8], const uint4 (&a)[LPM == 8 ? 2 : 1], const uint4 (&mask)[LPM == 8 ? 2 : 1],
                                             const float *rcp, const int *deq, int n_rungs, int lane, int *xw, unsigned long long *__restrict__ sums)
{
    constexpr int kPasses = LPM == 8 ? 2 : 1;
    const int slot = lane >> 3, i = lane & 7;
    uint32_t aa = 0;   // sum a^2: the same at every rung
#pragma unroll
    for (int pass = 0; pass < kPasses; pass++) aa = sq4(a[pass].x, a[pass].y, a[pass].z, a[pass].w, aa);
    for (int r = 0; r < n_rungs; r++) {
        uint32_t ab = 0, bb = 0;
#pragma unroll
        for (int pass = 0; pass < kPasses; pass++) {
            const uint4 b = and4(rd_recon_row<FLT>(nn[pass], rcp + 64 * r, deq + 64 * r, xw, slot, i), mask[pass]);
            ab = dot_ab(a[pass], b.x, b.y, b.z, b.w, ab);
            bb = sq4(b.x, b.y, b.z, b.w, bb);
        }
        rd_sse_out(aa + bb - 2u * ab, lane, &sums[(size_t)r * PITCH]);
    }
}

// Both table sets an i-frame uses (luma, chroma), reciprocals and dequantiser products (f32 bits in the float form: deq < 2^24, checked on the
// host) of all rungs: the workgroup's copy, made before any wavefront leaves (k_probe_iframe_rd, k_probe_iframe_ssim)
template <bool FLT>
__device__ __forceinline__ void rd_stage_intra_tables(const QTab *qtabs, int n_rungs, float (&rcp)[2][kProbeMaxRungs][64], int (&deq)[2][kProbeMaxRungs][64])
{
    for (int e = (int)threadIdx.x; e < n_rungs * 128; e += kThreads) {
        const int r = e >> 7, sel = (e >> 6) & 1, j = e & 63;
        const QTab *qt = qtabs + 4 * r + sel;
        rcp[sel][r][j] = qt->rcp[j];
        deq[sel][r][j] = FLT ? __float_as_int((float)qt->deq[j]) : qt->deq[j];
    }
    __syncthreads();
}

template <bool FLT, int LPM = 8>
__global__ __launch_bounds__(kThreads) void k_probe_iframe_rd(FrameGeom g, const uint8_t *__restrict__ src, const QTab *__restrict__ qtabs, int n_rungs,
                                                               uint32_t *__restrict__ acc, unsigned long long *__restrict__ sse_acc)
{
    __shared__ __attribute__((aligned(16))) int xchg[kStripsPerWG][kXchgDwords];
    __shared__ __attribute__((aligned(16))) int qtab_lds[kStripsPerWG][kQTabDwords];
    __shared__ float rcp_lds[2][kProbeMaxRungs][64];   // [luma, chroma]: intra_l / intra_c of every rung
    __shared__ int deq_lds[2][kProbeMaxRungs][64];
    constexpr int kPasses = LPM == 8 ? 2 : 1;

    rd_stage_intra_tables<FLT>(qtabs, n_rungs, rcp_lds, deq_lds);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gw = xcd_remap((int)blockIdx.x, (int)gridDim.x) * kStripsPerWG + wave;
    const int gstrip = LPM == 8 ? gw : gw >> 1, half_strip = LPM == 8 ? 0 : gw & 1;
    if (gstrip >= g.strips_per_frame * g.n_streams) return;   // no cross-wavefront sync from here on
    const StripPos sp = locate_strip(g, gstrip);
    if (half_strip * 4 >= sp.n_mb) return;
    const int m = LPM == 8 ? lane >> 3 : half_strip * 4 + (lane >> 4);   // macroblock within the strip
    fill_qtable<true, FLT>(qtab_lds[wave], qtabs + g.p[sp.plane].qsel, lane);
    const PlaneGeom &p = g.p[sp.plane];
    uint4 rows[kPasses], mask[kPasses];
    f2 nn[kPasses][8];
    int zz[8];
#pragma unroll
    for (int pass = 0; pass < kPasses; pass++) mask[pass] = rd_picture_mask(p, sp.x0 + m * 16, probe_strip_y<LPM>(sp, lane, pass));
    probe_strip_front<FLT, LPM>(g, src, sp, m, lane, qtab_lds[wave], xchg[wave], rows, nn, zz);
    const bool present = m < sp.n_mb;   // macroblocks beyond the strip's end count nothing (and lie outside the picture: their mask is empty)
    probe_rung_loop<LPM, kProbeAcc, kProbeStats>(nn, zz, &rcp_lds[p.qsel][0][0], n_rungs, lane, acc + (size_t)sp.stream * n_rungs * kProbeAcc,
                                                 [&](int) { return present; });
#pragma unroll
    for (int pass = 0; pass < kPasses; pass++) rows[pass] = and4(rows[pass], mask[pass]);
    rd_rung_loop<FLT, LPM, 3>(nn, rows, mask, &rcp_lds[p.qsel][0][0], &deq_lds[p.qsel][0][0], n_rungs, lane, xchg[wave],
                              sse_acc + ((size_t)sp.stream * n_rungs) * 3 + sp.plane);
}

// the three plane sums of the wavefront's (stream, rung) moved to the caller's buffer and cleared: the tail of both *_rd_sizes kernels
__device__ __forceinline__ void rd_sums_out(unsigned long long *__restrict__ sse_acc, unsigned long long *__restrict__ sse)
{
    const size_t at = (size_t)blockIdx.x * 3 + threadIdx.x;
    if (threadIdx.x < 3) {
        sse[at] = sse_acc[at];
        sse_acc[at] = 0;   // consumed: the next call starts clean
    }
}

// One wavefront per (stream, rung): k_probe_sizes's row, then the plane sums of the same (stream, rung) out and cleared
__global__ __launch_bounds__(64) void k_probe_rd_sizes(uint32_t *__restrict__ acc, uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats,
                                                       unsigned long long *__restrict__ sse_acc, unsigned long long *__restrict__ sse)
{
    __shared__ int32_t hist[16];
    __shared__ uint32_t val[16];
    __shared__ uint8_t len[16], table[16];
    __shared__ int parent[32], branch[32];
    probe_sizes_row<false>(acc, sizes, stats, hist, table, val, len, parent, branch);
    rd_sums_out(sse_acc, sse);
}

}  // namespace pfv
