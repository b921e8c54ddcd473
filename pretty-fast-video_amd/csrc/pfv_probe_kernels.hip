// pfv_probe_kernels.hip -- the i-frame size probe (gfx950): the payload size of a frame as an i-frame at EVERY rung of a session's quality
// ladder, from one read of the frame.
//
// A payload's size is a closed function of seventeen integers (k_ent_codes): bytes = (19 * 8 + sum_k hist[k] * len[k] + sumsize + 7) >> 3, with
// hist the 16-bin symbol histogram of rle_encode + update_table (src/rle.rs:9-47), len the code lengths of the reference's tree over the
// normalised histogram (rle.rs:49-66, src/huffman.rs:71-119) and sumsize the sum of coeff_size over the non-zero values.  The source read, the
// pixel bias, both 1-D transforms and the DCT_SCALE_FACTOR multiply (quant_scale) do not depend on the rung; only trunc(n * rcp) does.
//
//   probe_forward_row   one half-macroblock: unpack, (px - 128) << 8 (or the halved residual), rows, transpose, columns, quant_scale.  The
//                   forward half of the closed loop, once for all six probe kernels and both arithmetics.
//   probe_strip_front   the front end of the three i-frame kernels behind their strip mapping (k_enc_iframe's: one wavefront = a strip of 8
//                   macroblocks, or half of one under the 16-lane mapping; the two early-outs stay in the kernels): source rows, scaled
//                   coefficients, zigzag positions.
//   k_probe_iframe  the mapping and the front end -- the scaled coefficients of the lane's subblocks stay in registers (as floats: |n| <= 5160).  Then per
//                   rung r, with the reciprocals of all rungs staged in LDS once per wavefront:
//                     per value   q = trunc(n * rcp) (quant_div); e = q's exponent field: q != 0 <=> e != 0, coeff_size = bit length + 1 =
//                                 e - 125.  One bit into the lane's part of the subblock's 64-bit non-zero map at the value's zigzag position,
//                                 one count into a 64-bit word of sixteen 4-bit fields (a lane holds 8 values of a subblock), max(e) for the
//                                 oversize flag.  No coefficient is stored, no inverse transform runs.
//                     per macroblock  the parts are ORed over the macroblock's lanes (DPP); lane j then owns word j of the 256-bit map and
//                                 counts the runs that END in its word, bit-parallel: with S_k = the map shifted up by k, a value is preceded
//                                 by exactly r zeros where map & S_(r+1) & ~(S_1 | ... | S_r), r = 0..15 -- sixteen popcounts.  Position -1
//                                 counts as set (a run starts at the macroblock, enc.rs:246-255).  A value behind 16 or more zeros (at most
//                                 two per word) takes a loop: run length from the last set bit before it (prefix maximum over the lanes),
//                                 fillers and rest as ent_split_run; the closing run likewise, once per macroblock.
//                     per wavefront  the lanes' counts -- sixteen 8-bit fields, sizes and runs together; sumsize = four v_dot4 over the size
//                                 fields -- are widened to 16-bit fields, summed over each 16-lane row with DPP and over the four rows on the
//                                 scalar side, and seventeen lanes add them to acc[stream][rung] with one vector atomic.
//   probe_rung_loop the "per rung" part above as a device function: the p-frame probes (pfv_pprobe_kernels.hip) run it on residuals.
//   k_probe_sizes   one wavefront per (stream, rung): ent_build_codes_wave on the 16 counts, the size, and the accumulator cleared for the next
//                   call -- so a call needs no host-side clear and no host synchronisation, and a recorded pair of launches can be replayed.
// Included by pfv_capi.hip behind pfv_entropy_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfv {

constexpr int kProbeMaxRungs = 11;     // a ladder has at most this many rungs (pfv_enc_session_create_ladder)
constexpr int kProbeStats = 17;        // per (stream, rung): 16 symbol counts + the sum of coefficient sizes
constexpr int kProbeAcc = 18;          // the accumulator's row: the same + the oversize flag
// the p-frame probe's row: the same counts + coded macroblocks, macroblocks with a non-zero vector, block-header bits; then the oversize flag
constexpr int kPProbeStats = 20, kPProbeAcc = 21, kPProbeCodedAt = 17, kPProbeMovedAt = 18, kPProbeHdrAt = 19;
constexpr uint32_t kProbeOversizeExp = 127u + 14u;   // |q| >= 2^14: coeff_size >= 16 (rle.rs:44 would panic; kEntErrOversize)
constexpr uint64_t kNibbleEven = 0x0f0f0f0f0f0f0f0full;

template <int N>
__device__ __forceinline__ int probe_row_shr(int old, int v)   // DPP row_shr:N, lanes without a source keep `old`
{
    return __builtin_amdgcn_update_dpp(old, v, 0x110 + N, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t probe_mb_or(uint32_t v)    // OR over the 8 lanes of a slot
{
    v |= (uint32_t)dpp<kQuadXor1>((int)v);
    v |= (uint32_t)dpp<kQuadXor2>((int)v);
    v |= (uint32_t)dpp<kRowHalfMirror>((int)v);
    return v;
}

// Run symbols of one macroblock from its 256-bit non-zero map (words[j]: positions 32 j .. 32 j + 31 in coefficient order, the same in all of
// the macroblock's lanes): num_zeroes counts, fillers and the closing run, added to the lane's sixteen 8-bit counters -- ev: bins 0, 2, .. 14 in
// bytes 0..7, od: bins 1, 3, .. 15.  LPM = 8: the macroblock's 8 lanes take a word each; LPM = 16: the first 8 of its 16 lanes do.
template <int LPM>
__device__ __forceinline__ void probe_runs(const uint32_t (&words)[8], int lane, uint64_t &ev, uint64_t &od)
{
    const int idx = LPM == 8 ? (lane & 7) : (lane & 15);
    uint32_t W = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) W = idx == j ? words[j] : W;
    constexpr uint32_t kBefore = 0x80000000u;   // the word in front of the macroblock: only position -1, set
    uint32_t P = (uint32_t)probe_row_shr<1>((int)kBefore, (int)W);
    if (idx == 0) P = kBefore;                  // 8 lanes: the odd macroblocks of a DPP row start at lane 8
    // last set position up to and including the lane's word: inclusive prefix maximum over the macroblock's lanes
    const int base = 32 * idx;
    int incl = W ? base + 31 - __builtin_clz(W) : -1;
    {
        int t = probe_row_shr<1>(-1, incl);
        incl = max(incl, (LPM == 8 && idx < 1) ? -1 : t);
        t = probe_row_shr<2>(-1, incl);
        incl = max(incl, (LPM == 8 && idx < 2) ? -1 : t);
        t = probe_row_shr<4>(-1, incl);
        incl = max(incl, (LPM == 8 && idx < 4) ? -1 : t);
        if (LPM == 16) incl = max(incl, probe_row_shr<8>(-1, incl));
    }
    int before = probe_row_shr<1>(-1, incl);    // ... and before the lane's word
    if (idx == 0) before = -1;

    // values preceded by exactly r zeros, r = 0..15: S holds the map shifted up by r + 1, O the OR of the shifts 1..r
    uint32_t O = 0, S = __builtin_amdgcn_alignbit(W, P, 31);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const uint64_t n = (uint64_t)__builtin_popcount(W & S & ~O);
        if (r & 1) od += n << (8 * (r >> 1));
        else ev += n << (8 * (r >> 1));
        O |= S;
        S = __builtin_amdgcn_alignbit(W, P, 30 - r);
    }
    // values behind 16 zeros or more, and the closing run: fillers (15, size 0) and what is left (ent_split_run)
    uint64_t rest4 = 0;     // sixteen 4-bit counters: at most two such values per word and one closing run
    uint32_t n_fill = 0, closing = 0;
    for (uint32_t L = W & ~O; L; L &= L - 1) {
        const int b = __builtin_ctz(L);
        const uint32_t below = W & ((1u << b) - 1u);
        const int prev = below ? base + 31 - __builtin_clz(below) : before;
        unsigned fillers, rest;
        ent_split_run((unsigned)(base + b - prev - 1), fillers, rest);
        n_fill += fillers;
        rest4 += 1ull << (4u * rest);
    }
    if (idx == (LPM == 8 ? 7 : 15) && incl < 255) {   // (rest, size 0) behind its fillers (rle.rs:31-38)
        unsigned fillers, rest;
        ent_split_run((unsigned)(255 - incl), fillers, rest);
        n_fill += fillers;
        rest4 += 1ull << (4u * rest);
        closing = 1;
    }
    ev += (rest4 & kNibbleEven) + n_fill + closing;   // bin 0: the size symbol of every filler and of the closing run
    od += ((rest4 >> 4) & kNibbleEven) + ((uint64_t)n_fill << 56);   // bin 15: the fillers
}

// The rung loop of the size probes (k_probe_iframe, k_probe_pframe): nn = the lane's scaled coefficients, zz = their zigzag positions, rcp = the
// reciprocals of all rungs [n_rungs][64] (LDS), rows = the accumulator rows of the wavefront's stream (PITCH words per rung, the oversize flag
// at word FLAG_AT); counts(r): the lane's macroblock is written at rung r (an i-frame: it exists; a p-frame: it exists and is coded there).
template <int LPM, int PITCH, int FLAG_AT, class Counts>
__device__ __forceinline__ void probe_rung_loop(const f2 (&nn)[LPM == 8 ? 2 : 1][8], const int (&zz)[8], const float *rcp, int n_rungs, int lane,
                                                uint32_t *__restrict__ rows, Counts &&counts)
{
    constexpr int kPasses = LPM == 8 ? 2 : 1;
    const int slot = lane >> 3, i = lane & 7;
    for (int r = 0; r < n_rungs; r++) {
        const float *rc = rcp + 64 * r;
        uint64_t nzmap[kPasses][2], size4[kPasses][2];   // per subblock: the lane's part of the non-zero map; sixteen 4-bit size counters
        uint32_t emax = 0;
#pragma unroll
        for (int pass = 0; pass < kPasses; pass++) {
            nzmap[pass][0] = nzmap[pass][1] = size4[pass][0] = size4[pass][1] = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const f2 q = f2trunc(nn[pass][k] * f2s(rc[k * 8 + i]));   // quant_div: n / q, truncating
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const uint32_t e = ((uint32_t)__float_as_int(q[s]) >> 23) & 0xffu;
                    const uint64_t nz = (uint64_t)min(e, 1u);
                    emax = max(emax, e);
                    nzmap[pass][s] |= nz << zz[k];
                    size4[pass][s] += nz << ((4u * e - 500u) & 63u);   // bin coeff_size = e - 125
                }
            }
        }
        // the macroblock's map in all of its lanes
        uint32_t words[8];
        if (LPM == 8) {
#pragma unroll
            for (int pass = 0; pass < kPasses; pass++)
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    words[4 * pass + 2 * s] = probe_mb_or((uint32_t)nzmap[pass][s]);
                    words[4 * pass + 2 * s + 1] = probe_mb_or((uint32_t)(nzmap[pass][s] >> 32));
                }
        } else {   // the slot holds subblocks 2h, 2h + 1; the other half lies 8 lanes away
            const bool upper = (slot & 1) != 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t mine = probe_mb_or((uint32_t)(nzmap[0][j >> 1] >> (32 * (j & 1))));
                const uint32_t other = (uint32_t)dpp<kRowRor8>((int)mine);
                words[j] = upper ? other : mine;
                words[4 + j] = upper ? mine : other;
            }
        }
        uint64_t ev = 0, od = 0;
#pragma unroll
        for (int pass = 0; pass < kPasses; pass++)
#pragma unroll
            for (int s = 0; s < 2; s++) {
                ev += size4[pass][s] & kNibbleEven;
                od += (size4[pass][s] >> 4) & kNibbleEven;
            }
        // sum of coeff_size: bin x count over the size counters alone, before the run symbols join them
        uint32_t sumsize = __builtin_amdgcn_udot4((uint32_t)ev, 0x06040200u, 0u, false);
        sumsize = __builtin_amdgcn_udot4((uint32_t)(ev >> 32), 0x0e0c0a08u, sumsize, false);
        sumsize = __builtin_amdgcn_udot4((uint32_t)od, 0x07050301u, sumsize, false);
        sumsize = __builtin_amdgcn_udot4((uint32_t)(od >> 32), 0x0f0d0b09u, sumsize, false);
        probe_runs<LPM>(words, lane, ev, od);
        const bool present = counts(r);
        if (!present) { ev = od = 0; sumsize = 0; }

        // 8-bit fields (a lane's count stays below 96) -> 16-bit fields (a wavefront's below 64 * 96), d[2 a + b]: bytes b and b + 2 of dword a
        const uint32_t x[4] = {(uint32_t)ev, (uint32_t)(ev >> 32), (uint32_t)od, (uint32_t)(od >> 32)};
        uint32_t tot[8];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const uint32_t d = ent_row_sum((x[a] >> (8 * b)) & 0x00ff00ffu);
                tot[2 * a + b] = (uint32_t)(__builtin_amdgcn_readlane((int)d, 0) + __builtin_amdgcn_readlane((int)d, 16) + __builtin_amdgcn_readlane((int)d, 32) +
                                            __builtin_amdgcn_readlane((int)d, 48));
            }
        const uint32_t ss = ent_row_sum(sumsize);
        const uint32_t ss_tot = (uint32_t)(__builtin_amdgcn_readlane((int)ss, 0) + __builtin_amdgcn_readlane((int)ss, 16) + __builtin_amdgcn_readlane((int)ss, 32) +
                                           __builtin_amdgcn_readlane((int)ss, 48));
        // lane k < 16: bin k = byte k / 2 of ev (k even) or od (k odd); lane 16: the size sum
        const int byte = lane >> 1, sel = (lane & 1) * 4 + (byte >> 2) * 2 + (byte & 1);
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) mine = sel == j ? tot[j] : mine;
        mine = (byte & 2) ? mine >> 16 : mine & 0xffffu;
        if (lane == 16) mine = ss_tot;
        uint32_t *row = rows + (size_t)r * PITCH;
        if (lane < kProbeStats && mine) atomicAdd(&row[lane], mine);
        if (__any(present && emax >= kProbeOversizeExp) && lane == 0) atomicOr(&row[FLAG_AT], 1u);
    }
}

// The forward half of the closed loop for one half-macroblock, rd_recon_row's mirror image (pfv_rdprobe_kernels.hip): row = the lane's 16 source
// pixels -> nn = (m * SCALE) >> 16 of its two subblocks in column layout, nn[k] = rows k of subblocks 2h and 2h + 1, column i.  An i-frame:
// (px - 128) << 8 (src/common.rs:291); RESIDUAL: calc_residuals against the prediction's row `pred` (:118-119), delta / 2 truncating, << 8
// (:304).  Rows, transpose through the macroblock's exchange region `mb`, columns, quant_scale: forward_half's / penc_half's arithmetic, FLT in f32.
template <bool FLT, bool RESIDUAL = false>
__device__ __forceinline__ void probe_forward_row(const uint4 &row, const uint4 &pred, int *mb, int i, int quarter, const LaneQ lq, f2 (&nn)[8])
{
    if (FLT) {
        f2 x[8], pp[8];
        unpack_row_f(row, x);
        if (RESIDUAL) unpack_row_f(pred, pp);
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = RESIDUAL ? residual_f(x[k], pp[k]) : x[k] * f2s(256.0f) - f2s(32768.0f);
        ffdct8(x);
        f_rows_to_cols(x, mb, i, quarter);
        ffdct8(x);
#pragma unroll
        for (int k = 0; k < 8; k++) nn[k] = quant_scale(x[k], lq.scale(k));
    } else {
        int v[2][8], pp[2][8];
        unpack_row(row, v);
        if (RESIDUAL) unpack_row(pred, pp);
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int k = 0; k < 8; k++) v[s][k] = (int)((unsigned)(RESIDUAL ? tdiv2(v[s][k] - pp[s][k]) : v[s][k] - 128) << 8);
        }
        fdct8(v[0]);
        fdct8(v[1]);
        rows_to_cols2(v, mb, i, quarter);
        fdct8(v[0]);
        fdct8(v[1]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int scale = lq.scale(k);
            nn[k] = f2{(float)(wmul24(v[0][k], scale) >> 16), (float)(wmul24(v[1][k], scale) >> 16)};
        }
    }
}

// the picture row of the lane's source row `pass` (its column is sp.x0 + m * 16)
template <int LPM>
__device__ __forceinline__ int probe_strip_y(const StripPos &sp, int lane, int pass)
{
    return sp.y0 + (lane & 7) + 8 * (LPM == 8 ? pass : ((lane >> 3) & 1));
}
// The strip probes' front end (k_probe_iframe, _rd, _ssim), behind the kernel's two early-outs: everything that does not depend on the rung.
// The early-outs stay in the kernels: reported through a helper, StripPos reaches this code through a phi and x0 loses its known-zero low bits
// (profiles/probe_front_refactor.md).  qtab = the wavefront's table entry, filled by the kernel (fill_qtable: scale and zigzag position; its
// reciprocal and dequantiser are rung 0's and are not used) like whatever else it stages per wavefront -- the wave_lds_sync in here publishes
// both.  xw = the wavefront's exchange region -> rows = the lane's source rows, nn = their scaled coefficients (probe_forward_row), zz = the
// zigzag positions of the lane's values.
// The order of the rung loops behind a front end is a register matter.  The source rows (and a p-frame's patch rows) end in the distortion
// loop; kept alive across probe_rung_loop they cost k_probe_pframe_rd (281 registers against 256) and the 8-lane k_probe_iframe_ssim (258) their
// second wavefront per SIMD.  So those two and k_probe_pframe_ssim run the distortion loop first, and the p-frame forms its picture masks
// behind the search; k_probe_iframe_rd fits either way and keeps the size loop first (profiles/pframe_rd_probe.md).
template <bool FLT, int LPM>
__device__ __forceinline__ void probe_strip_front(const FrameGeom &g, const uint8_t *src, const StripPos &sp, int m, int lane, const int *qtab, int *xw,
                                                  uint4 (&rows)[LPM == 8 ? 2 : 1], f2 (&nn)[LPM == 8 ? 2 : 1][8], int (&zz)[8])
{
    constexpr int kPasses = LPM == 8 ? 2 : 1;
    const PlaneGeom &p = g.p[sp.plane];
    const int slot = lane >> 3, i = lane & 7;
    const uint8_t *plane = frame_src(g, src, sp.stream) + p.src_off;
#pragma unroll
    for (int pass = 0; pass < kPasses; pass++) rows[pass] = load_src16(plane, p, sp.x0 + m * 16, probe_strip_y<LPM>(sp, lane, pass));
    wave_lds_sync();
    const LaneQ lq{qtab, i};
    int *mb = xw + slot * kMBPitch;
#pragma unroll
    for (int pass = 0; pass < kPasses; pass++) probe_forward_row<FLT>(rows[pass], uint4(), mb, i, slot & 3, lq, nn[pass]);
#pragma unroll
    for (int k = 0; k < 8; k++) zz[k] = lq.zz(k);
}

template <bool FLT, int LPM = 8>
__global__ __launch_bounds__(kThreads) void k_probe_iframe(FrameGeom g, const uint8_t *__restrict__ src, const QTab *__restrict__ qtabs, int n_rungs,
                                                            uint32_t *__restrict__ acc)
{
    __shared__ __attribute__((aligned(16))) int xchg[kStripsPerWG][kXchgDwords];
    __shared__ __attribute__((aligned(16))) int qtab_lds[kStripsPerWG][kQTabDwords];
    __shared__ float rcp_lds[kStripsPerWG][kProbeMaxRungs][64];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gw = xcd_remap((int)blockIdx.x, (int)gridDim.x) * kStripsPerWG + wave;
    const int gstrip = LPM == 8 ? gw : gw >> 1, half_strip = LPM == 8 ? 0 : gw & 1;
    if (gstrip >= g.strips_per_frame * g.n_streams) return;   // no cross-wavefront sync from here on
    const StripPos sp = locate_strip(g, gstrip);
    if (half_strip * 4 >= sp.n_mb) return;
    const int m = LPM == 8 ? lane >> 3 : half_strip * 4 + (lane >> 4);   // macroblock within the strip
    fill_qtable<true, FLT>(qtab_lds[wave], qtabs + g.p[sp.plane].qsel, lane);
    // the reciprocals of all rungs, per wavefront and for its plane: intra_l / intra_c of rung r
    for (int r = 0; r < n_rungs; r++) rcp_lds[wave][r][lane] = qtabs[4 * r + g.p[sp.plane].qsel].rcp[lane];
    uint4 rows[LPM == 8 ? 2 : 1];
    f2 nn[LPM == 8 ? 2 : 1][8];
    int zz[8];
    probe_strip_front<FLT, LPM>(g, src, sp, m, lane, qtab_lds[wave], xchg[wave], rows, nn, zz);
    const bool present = m < sp.n_mb;   // macroblocks beyond the strip's end count nothing
    probe_rung_loop<LPM, kProbeAcc, kProbeStats>(nn, zz, &rcp_lds[wave][0][0], n_rungs, lane, acc + (size_t)sp.stream * n_rungs * kProbeAcc,
                                                 [&](int) { return present; });
}

// One wavefront per (stream, rung): acc rows in, sizes (and the counts, where asked for) out, acc rows cleared.  PFRAME: the rows of
// k_probe_pframe (pfv_pprobe_kernels.hip) -- three more counts, of which the block-header bits join the size.  The body of both kernels; the LDS
// arrays are theirs (function-local to a plain kernel, so the compiler can drop the ones ent_build_codes_wave only writes).
template <bool PFRAME>
__device__ __forceinline__ void probe_sizes_row(uint32_t *__restrict__ acc, uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats, int32_t *hist, uint8_t *table,
                                                uint32_t *val, uint8_t *len, int *parent, int *branch)
{
    constexpr int kAcc = PFRAME ? kPProbeAcc : kProbeAcc, kStats = PFRAME ? kPProbeStats : kProbeStats;
    const int lane = (int)threadIdx.x;
    const size_t e = blockIdx.x;
    uint32_t *row = acc + e * kAcc;
    uint32_t mine = 0;
    if (lane < kAcc) {
        mine = row[lane];
        row[lane] = 0;   // consumed: the next call starts clean
    }
    if (lane < 16) hist[lane] = (int32_t)mine;
    if (stats && lane < kStats) stats[e * kStats + lane] = mine;
    ent_wave_lds_sync();
    ent_build_codes_wave(hist, table, val, len, parent, branch);
    ent_wave_lds_sync();
    const uint32_t bits = ent_wave_sum(lane < 16 ? mine * (uint32_t)len[lane] : 0u);
    const uint32_t sumsize = ent_shfl(mine, 16), oversize = ent_shfl(mine, kStats);
    const uint32_t hdr_bits = PFRAME ? ent_shfl(mine, kPProbeHdrAt) : 0u;   // 2 per macroblock, 16 where the vector is non-zero (k_ent_scan)
    if (lane == 0) sizes[e] = oversize ? kEntErrOversize : (19u * 8u + hdr_bits + bits + sumsize + 7u) >> 3;   // as k_ent_codes: 16 table bytes + 3 q indices first
}
__global__ __launch_bounds__(64) void k_probe_sizes(uint32_t *__restrict__ acc, uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats)
{
    __shared__ int32_t hist[16];
    __shared__ uint32_t val[16];
    __shared__ uint8_t len[16], table[16];
    __shared__ int parent[32], branch[32];
    probe_sizes_row<false>(acc, sizes, stats, hist, table, val, len, parent, branch);
}
__global__ __launch_bounds__(64) void k_pprobe_sizes(uint32_t *__restrict__ acc, uint32_t *__restrict__ sizes, uint32_t *__restrict__ stats)
{
    __shared__ int32_t hist[16];
    __shared__ uint32_t val[16];
    __shared__ uint8_t len[16], table[16];
    __shared__ int parent[32], branch[32];
    probe_sizes_row<true>(acc, sizes, stats, hist, table, val, len, parent, branch);
}

}  // namespace pfv
