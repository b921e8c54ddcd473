// pfv_ssimprobe_kernels.hip -- the SSIM probe (gfx950): payload size, squared error AND the SSIM sums of a frame as an i-frame or as a p-frame
// at EVERY rung of a session's quality ladder, from one read of the frame (one search and one forward transform for a p-frame).
//
// An SSIM window (pfv_ssim_kernels.hip) is 2 x 2 blocks of 4 x 4 pixels, so the 16 windows of a macroblock need the block column of the
// macroblock to its right and the block row of the strip below.  In a probe the reconstruction at rung r exists only in the registers of the
// wavefront that rebuilt it, and the p-frame probe's tile form does not keep neighbouring macroblocks in neighbouring wavefronts.  So the
// probe kernels leave the 4 x 4 BLOCK SUMS of every rung in a map in scratch, and a second kernel forms the windows from it:
//
//   k_probe_iframe_ssim   rd_stage_intra_tables, probe_strip_front (both lane mappings), probe_rung_loop.  Its distortion loop per rung: the
//                         reconstructed row of rd_recon_row, masked like the source row (rd_picture_mask), then per dword -- one block-row --
//                         v_dot4_u32_u8 once each for sum b, sum b^2 and sum ab.  sum b (<= 4080) and sum b^2 (<= 1 040 400) of a block share
//                         a dword (12 + 20 bits), sum ab (<= 1 040 400) takes the next.  The lane's squared error is the sum of the same terms,
//                         sum a^2 - 2 sum ab + sum b^2: no second pass over the row.  The four rows of a block lie in the four lanes of a quad:
//                         quad_col_sum adds them with three DPP moves per four columns and leaves column j in lane j of the quad.
//                         8 lanes per macroblock: a lane then holds blocks (i >> 2, i & 3) and ((i >> 2) + 2, i & 3) and stores their four
//                         dwords with ONE 16-byte store at [stream][rung][macroblock][lane i] -- a strip writes 1 KiB contiguous per rung.
//                         16 lanes: one block per lane, the same place, 8 bytes.  The source's sum a | sum a^2 << 12 do not depend on the rung:
//                         one dword per block, [stream][macroblock][16], stored once.
//                         The masks cost the block sums nothing: a window exists only when all 64 of its pixels lie inside the picture (the
//                         argument at the head of k_ssim_mb), so a block that the mask touches belongs to no window.
//   k_probe_pframe_ssim   the same behind probe_tile_front<FLT, true> (8 lanes per macroblock only).  A macroblock skipped at rung r stores
//                         the block sums of its patch, formed once before the rung loop like skip_sse; a coded one those of
//                         rd_recon_row<FLT, true>.  The wavefront-uniform early-out of a rung at which nothing is coded stays; the stores happen.
//   k_probe_ssim_windows  one workgroup per (stream of the window, rung); 8 lanes per macroblock of the frame (all planes) read the map back as it
//                         was written and gather the blocks of two windows each -- neighbours through the plane's macroblock grid, so across
//                         strips and tiles --, add 2 x 2 of them per window that exists (bx + 1 < w >> 2, by + 1 < h >> 2) and call k_ssim_mb's
//                         own ssim_window_q24 on the same integers.  Sums per plane in 64 bits through a FIXED reduction (k_ssim_sum's), written
//                         straight to ssim_q24[stream][rung][plane]: no accumulator, nothing to clear, replays from a graph.
// Sizes, counts and the plane sums of the squared error leave through the RD probes' own tail, UNCHANGED and as the launch group's third launch:
// k_probe_rd_sizes / k_pprobe_rd_sizes (the accumulators are the RD probes').
//
// Map bytes per stream: mbs_per_frame * (n_rungs * 128 + 64).
// Included by pfv_capi.hip behind pfv_prdprobe_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfv {

constexpr int kSsimMapRec = 32;   // dwords per macroblock and rung: 16 blocks x (sum b | sum b^2 << 12, sum ab)
constexpr int kSsimMapSrc = 16;   // dwords per macroblock: 16 blocks x (sum a | sum a^2 << 12)
// dwords of one stream's map: the source's sums, then the rungs'
__host__ __device__ inline size_t ssim_map_stream_dwords(int mbs_per_frame, int n_rungs) { return (size_t)mbs_per_frame * (size_t)(kSsimMapSrc + kSsimMapRec * n_rungs); }

// one block-row (a dword of four pixels): sum x | sum x^2 << 12; the fields hold a whole block's sums, so the quad's sum carries nothing across
__device__ __forceinline__ unsigned ssim_pack_row(unsigned x, unsigned &sq)
{
    sq = __builtin_amdgcn_udot4(x, x, 0u, false);
    return __builtin_amdgcn_udot4(x, 0x01010101u, sq << 12, false);
}
// v[d]: the lane's value for block column d -> the sum of column j = lane & 3 over the four lanes of the quad (quad_sum's moves, but each
// step sends the half the receiver keeps: 3 DPP moves instead of 8)
__device__ __forceinline__ unsigned quad_col_sum(const unsigned (&v)[4], int j)
{
    const bool b1 = (j & 2) != 0, b0 = (j & 1) != 0;
    unsigned k2[2];
#pragma unroll
    for (int k = 0; k < 2; k++) k2[k] = (b1 ? v[2 + k] : v[k]) + (unsigned)dpp<kQuadXor2>((int)(b1 ? v[k] : v[2 + k]));
    return (b0 ? k2[1] : k2[0]) + (unsigned)dpp<kQuadXor1>((int)(b0 ? k2[0] : k2[1]));
}
// The block sums of one masked row pair (a = source, b = reconstruction): w0 / w1 = the two dwords of the lane's block after the quad's sum;
// ab / bb: the lane's own sum ab and sum b^2 are added (its share of the squared error)
__device__ __forceinline__ void ssim_rec_row(const uint4 &a, const uint4 &b, int j, unsigned &w0, unsigned &w1, unsigned &ab, unsigned &bb)
{
    const unsigned av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    unsigned p0[4], p1[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        unsigned sq;
        p0[d] = ssim_pack_row(bv[d], sq);
        p1[d] = __builtin_amdgcn_udot4(av[d], bv[d], 0u, false);
        bb += sq;
        ab += p1[d];
    }
    w0 = quad_col_sum(p0, j);
    w1 = quad_col_sum(p1, j);
}
// ... and of a masked source row alone: the lane's block's dword; aa: the lane's sum a^2 is added
__device__ __forceinline__ unsigned ssim_src_row(const uint4 &a, int j, unsigned &aa)
{
    const unsigned av[4] = {a.x, a.y, a.z, a.w};
    unsigned p0[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        unsigned sq;
        p0[d] = ssim_pack_row(av[d], sq);
        aa += sq;
    }
    return quad_col_sum(p0, j);
}

template <bool FLT, int LPM = 8>
__global__ __launch_bounds__(kThreads) void k_probe_iframe_ssim(FrameGeom g, const uint8_t *__restrict__ src, const QTab *__restrict__ qtabs, int n_rungs,
                                                                 uint32_t *__restrict__ acc, unsigned long long *__restrict__ sse_acc, uint32_t *__restrict__ map)
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
    const int slot = lane >> 3, i = lane & 7;
    int *xw = xchg[wave];
    uint4 rows[kPasses], mask[kPasses];
    f2 nn[kPasses][8];
    int zz[8];
    probe_strip_front<FLT, LPM>(g, src, sp, m, lane, qtab_lds[wave], xw, rows, nn, zz);
    const bool present = m < sp.n_mb;   // macroblocks beyond the strip's end count nothing and store nothing
    // distortion and block sums, in front of the size loop.  The lane's place in a macroblock's part of the map: 4 dwords per lane i, of which
    // the 16-lane mapping's second row half (slot & 1: block rows 2 and 3) takes the upper two
    const size_t mbs = (size_t)g.mbs_per_frame, mbi = (size_t)(sp.mb_first + m);
    uint32_t *smap = map + (size_t)sp.stream * ssim_map_stream_dwords(g.mbs_per_frame, n_rungs);
    uint32_t *src_at = smap + mbi * kSsimMapSrc + i * 2 + (LPM == 8 ? 0 : (slot & 1));
    uint32_t *rec_at = smap + mbs * kSsimMapSrc + mbi * kSsimMapRec + i * 4 + (LPM == 8 ? 0 : 2 * (slot & 1));
    uint32_t aa = 0;
    uint32_t sw[kPasses];
#pragma unroll
    for (int pass = 0; pass < kPasses; pass++) {
        mask[pass] = rd_picture_mask(p, sp.x0 + m * 16, probe_strip_y<LPM>(sp, lane, pass));
        rows[pass] = and4(rows[pass], mask[pass]);
        sw[pass] = ssim_src_row(rows[pass], i & 3, aa);
    }
    if (present) {
        if (LPM == 8) *reinterpret_cast<uint2 *>(src_at) = make_uint2(sw[0], sw[kPasses - 1]);
        else *src_at = sw[0];
    }
    unsigned long long *sums = sse_acc + ((size_t)sp.stream * n_rungs) * 3 + sp.plane;
    const float *rcp = &rcp_lds[p.qsel][0][0];
    const int *deq = &deq_lds[p.qsel][0][0];
    for (int r = 0; r < n_rungs; r++) {
        uint32_t ab = 0, bb = 0, w[kPasses][2];
#pragma unroll
        for (int pass = 0; pass < kPasses; pass++) {
            const uint4 b = and4(rd_recon_row<FLT>(nn[pass], rcp + 64 * r, deq + 64 * r, xw, slot, i), mask[pass]);
            ssim_rec_row(rows[pass], b, i & 3, w[pass][0], w[pass][1], ab, bb);
        }
        if (present) {
            uint32_t *at = rec_at + (size_t)r * mbs * kSsimMapRec;
            if (LPM == 8) *reinterpret_cast<uint4 *>(at) = make_uint4(w[0][0], w[0][1], w[kPasses - 1][0], w[kPasses - 1][1]);
            else *reinterpret_cast<uint2 *>(at) = make_uint2(w[0][0], w[0][1]);
        }
        rd_sse_out(aa + bb - 2u * ab, lane, &sums[(size_t)r * 3]);
    }
    probe_rung_loop<LPM, kProbeAcc, kProbeStats>(nn, zz, rcp, n_rungs, lane, acc + (size_t)sp.stream * n_rungs * kProbeAcc, [&](int) { return present; });
}

template <bool FLT>
__global__ __launch_bounds__(kThreads) void k_probe_pframe_ssim(FrameGeom g, const uint8_t *__restrict__ src, const uint8_t *__restrict__ ref,
                                                                 const QTab *__restrict__ qtabs, int n_rungs, const float *__restrict__ min_err, int neg2,
                                                                 uint32_t *__restrict__ acc, unsigned long long *__restrict__ sse_acc, uint32_t *__restrict__ map)
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
    const bool mb_valid = m < cur.sp.n_mb;   // macroblocks beyond the strip's end count nothing and store nothing
    const float err = (float)so.err;
    const auto coded_at = [&](int r) { return mb_valid && !(err <= err_lds[r]); };   // the skip decision (:209, :221) at rung r

    // distortion and block sums, in front of the size loop.  The patch's block sums and squared error are the same at every rung: what a
    // skipped macroblock stores and adds
    const size_t mbs = (size_t)g.mbs_per_frame, mbi = (size_t)(cur.sp.mb_first + m);
    uint32_t *smap = map + (size_t)cur.sp.stream * ssim_map_stream_dwords(g.mbs_per_frame, n_rungs);
    uint32_t *rec_at = smap + mbs * kSsimMapSrc + mbi * kSsimMapRec + i * 4;
    uint4 mask[2];
    uint32_t aa = 0, skip_ab = 0, skip_bb = 0, sw[2], skip_w[2][2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        mask[h] = rd_picture_mask(p, cur.sp.x0 + m * 16, cur.sp.y0 + i + 8 * h);
        rows[h] = and4(rows[h], mask[h]);
        sw[h] = ssim_src_row(rows[h], i & 3, aa);
        ssim_rec_row(rows[h], and4(so.patch[h], mask[h]), i & 3, skip_w[h][0], skip_w[h][1], skip_ab, skip_bb);
    }
    if (mb_valid) *reinterpret_cast<uint2 *>(smap + mbi * kSsimMapSrc + i * 2) = make_uint2(sw[0], sw[1]);
    const uint32_t skip_sse = aa + skip_bb - 2u * skip_ab;
    unsigned long long *sums = sse_acc + ((size_t)cur.sp.stream * n_rungs) * 3 + cur.sp.plane;
    for (int r = 0; r < n_rungs; r++) {
        const bool coded = coded_at(r);
        uint32_t lane_sse = skip_sse;
        uint4 out = make_uint4(skip_w[0][0], skip_w[0][1], skip_w[1][0], skip_w[1][1]);
        if (__ballot(coded) != 0ull) {   // wavefront-uniform: the transposes and the quads' sums below need all 64 lanes
            uint32_t ab = 0, bb = 0, w[2][2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint4 b = and4(rd_recon_row<FLT, true>(nn[h], &rcp_lds[r][0], &deq_lds[r][0], xw, m, i, so.patch[h]), mask[h]);
                ssim_rec_row(rows[h], b, i & 3, w[h][0], w[h][1], ab, bb);
            }
            if (coded) {
                lane_sse = aa + bb - 2u * ab;
                out = make_uint4(w[0][0], w[0][1], w[1][0], w[1][1]);
            }
        }
        if (mb_valid) *reinterpret_cast<uint4 *>(rec_at + (size_t)r * mbs * kSsimMapRec) = out;
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

// The two blocks lane `li` of the 8-lane mapping stored for macroblock `at` -- (li >> 2, li & 3) and ((li >> 2) + 2, li & 3) -- as window
// operands: sum a in the low and sum b in the high half of s (ssim_block_row's packing), sum a^2 + sum b^2, sum ab.  !ok: nothing is read.
__device__ __forceinline__ void ssim_map_blocks(const uint32_t *smap, const uint32_t *rmap, size_t at, int li, bool ok, SsimSums &b0, SsimSums &b1)
{
    uint2 a = make_uint2(0u, 0u);
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    if (ok) {
        a = *reinterpret_cast<const uint2 *>(smap + at * kSsimMapSrc + li * 2);
        b = *reinterpret_cast<const uint4 *>(rmap + at * kSsimMapRec + li * 4);
    }
    b0 = SsimSums{(int)((a.x & 0xfffu) | ((b.x & 0xfffu) << 16)), (int)((a.x >> 12) + (b.x >> 12)), (int)b.y};
    b1 = SsimSums{(int)((a.y & 0xfffu) | ((b.z & 0xfffu) << 16)), (int)((a.y >> 12) + (b.z >> 12)), (int)b.w};
}
// ... and the first of them alone (a block of block row 0 or 1)
__device__ __forceinline__ SsimSums ssim_map_block(const uint32_t *smap, const uint32_t *rmap, size_t at, int li, bool ok)
{
    unsigned a = 0u;
    uint2 b = make_uint2(0u, 0u);
    if (ok) {
        a = smap[at * kSsimMapSrc + li * 2];
        b = *reinterpret_cast<const uint2 *>(rmap + at * kSsimMapRec + li * 4);
    }
    return SsimSums{(int)((a & 0xfffu) | ((b.x & 0xfffu) << 16)), (int)((a >> 12) + (b.x >> 12)), (int)b.y};
}

// One workgroup per (stream, rung): blockIdx.x = stream * n_rungs + rung; map: the first stream's; ssim: [stream][rung][3].
// The probes' own lane mapping reads the map back: 8 lanes per macroblock, lane i = (quad, j) takes the 16 bytes lane i stored -- a wavefront
// reads 1 KiB contiguous per load, where a thread per macroblock strode 128 bytes and lost every line before it came back to it (that form took
// 6.4 ms for 96 x 1080p x 11 rungs against 0.96 for 5: the lines in use outgrew the L2, profiles/ssim_probe.md).  The lane adds the block column to its right (lane i + 1,
// or lane (quad, 0) of the next macroblock) and holds column pair j of block rows quad and quad + 2; block row 4 is row 0 of the macroblock
// below.  From there on it is k_ssim_mb: one exchange with the other quad gives the lane two vertically neighbouring windows.
__global__ __launch_bounds__(kThreads) void k_probe_ssim_windows(FrameGeom g, int n_rungs, const uint32_t *__restrict__ map, int64_t *__restrict__ ssim)
{
    __shared__ long long part[3][kStripsPerWG];
    const int stream = (int)blockIdx.x / n_rungs, r = (int)blockIdx.x - stream * n_rungs;
    const uint32_t *smap = map + (size_t)stream * ssim_map_stream_dwords(g.mbs_per_frame, n_rungs);
    const uint32_t *rmap = smap + (size_t)g.mbs_per_frame * kSsimMapSrc + (size_t)r * g.mbs_per_frame * kSsimMapRec;
    const int i = (int)threadIdx.x & 7, quad = i >> 2, j = i & 3;
    long long acc[3] = {0, 0, 0};
    for (int base = 0; base < g.mbs_per_frame; base += kThreads / 8) {   // the same trip count in every lane: the exchange needs whole quads
        const int k = base + ((int)threadIdx.x >> 3);
        const bool mb_ok = k < g.mbs_per_frame;
        const int kk = mb_ok ? k : 0;
        const int plane = (g.n_planes > 2 && kk >= g.p[2].mb0) ? 2 : ((g.n_planes > 1 && kk >= g.p[1].mb0) ? 1 : 0);
        const PlaneGeom &p = g.p[plane];
        const int local = kk - p.mb0, mby = local / p.bw, mbx = local - mby * p.bw;
        const int nbw = p.w >> 2, nbh = p.h >> 2;   // whole blocks of the picture
        // macroblocks that do not exist are not read: no window that exists needs them
        const bool right_ok = mb_ok && (j < 3 || mbx + 1 < p.bw), below_ok = mb_ok && quad && mby + 1 < p.bh;   // only quad 1 uses block row 4
        const size_t right_at = (size_t)(j < 3 ? kk : kk + 1), below_at = (size_t)(kk + p.bw);
        SsimSums own[2], right[2];
        ssim_map_blocks(smap, rmap, (size_t)kk, i, mb_ok, own[0], own[1]);
        ssim_map_blocks(smap, rmap, right_at, j < 3 ? i + 1 : quad * 4, right_ok, right[0], right[1]);
        const SsimSums below = ssim_map_block(smap, rmap, below_at, j, below_ok);
        const SsimSums below_right = ssim_map_block(smap, rmap, j < 3 ? below_at : below_at + 1, j < 3 ? j + 1 : 0, below_ok && right_ok);
        // column pair j of block rows quad, quad + 2 and 4
        const SsimSums h[3] = {own[0] + right[0], own[1] + right[1], below + below_right};
        const SsimSums send = quad ? h[0] : h[1];
        const SsimSums got = SsimSums{other_quad(send.s), other_quad(send.ss), other_quad(send.s12)};
        const SsimSums win0 = got + (quad ? h[1] : h[0]), win1 = h[1] + (quad ? h[2] : got);
        const int bx = mbx * 4 + j, by = mby * 4 + 2 * quad;
        int q = 0;
        if (mb_ok && bx + 1 < nbw) {
            if (by + 1 < nbh) q += ssim_window_q24(win0);
            if (by + 2 < nbh) q += ssim_window_q24(win1);
        }
        acc[plane] += q;   // two windows: |q| <= 2^25
    }
#pragma unroll
    for (int pl = 0; pl < 3; pl++) {
        long long v = acc[pl];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {   // two's complement: the halves travel as bits (k_ssim_sum)
            const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)v, off);
            const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v >> 32), off);
            v = (long long)((unsigned long long)v + (((unsigned long long)hi << 32) | lo));
        }
        if ((threadIdx.x & 63) == 0) part[pl][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long total = 0;
#pragma unroll
        for (int w = 0; w < kStripsPerWG; w++) total += part[threadIdx.x][w];
        ssim[(size_t)blockIdx.x * 3 + threadIdx.x] = total;
    }
}

}  // namespace pfv
