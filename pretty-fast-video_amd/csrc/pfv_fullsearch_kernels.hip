// pfv_fullsearch_kernels.hip -- k_pf_search_full: exhaustive motion search of a p-frame (PFV_SEARCH_FULL, include/pfv_hip_ext.h).
// Included by pfv_capi.hip behind pfv_kernels.hip, whose tile decomposition, window DMA and source loads it uses.
//
// k_pf_search's outward contract: one workgroup per 128 x 64 tile, the +-15 / +-16 reference window staged by issue_window behind one barrier,
// motion vectors and flags out, a SKIPPED macroblock finished here (penc_store_skipped), a coded one left to k_pf_transform, which the host
// launches right behind it.  What differs is the search: every (dx, dy) with |dx|, |dy| <= R inside the padded plane, and the lexicographic
// minimum of (E, |dx| + |dy|, dy, dx) instead of the reference's four-step descent.
//
// Mapping ("candidate owner"): lane (m, i) owns the COLUMNS dx = -R + i + 8k (k = 0 .. ceil((2R + 1) / 8) - 1) of macroblock m's candidate
// square and keeps all 16 source rows of the macroblock in registers (64 VGPRs, handed round the macroblock's 8 lanes through LDS once).
// For one column it walks down the 2R + 16 window rows the column's candidates cover.  A row is read once (5 aligned dwords), shifted to
// the column's byte phase once (4 v_alignbyte) and squared once (4 v_dot4); it is row j of the candidate that started j rows above, for
// j = 0 .. 15, so 16 running sums of a.b move down a register chain -- acc[j] = acc[j - 1] + src[j] . row, which v_dot4's separate
// accumulator operand does without a move -- and the sum that leaves acc[15] is the finished  sum ab  of candidate dy = row - 15.  Its
// sum b^2  is the difference of two prefix sums of the row squares; the prefix of 16 rows ago comes out of a 16-entry ring in LDS (one
// ds_write_b32 and one ds_read_b32 per row, lane-linear: conflict-free).  E = sum a^2 - 2 sum ab + sum b^2 is exact in u32 (< 2^24).
// No partial sum ever leaves its lane; the lanes' best 64-bit keys meet in one three-step DPP minimum per macroblock.
// A column walks 2R + 16 rows for 2R + 1 candidates because the chain fills and drains: the first and the last 15 rows are unrolled with
// the chain's live slots as compile-time bounds, so the products issued are the 16 x 4 per candidate and no more.
//
// Resources (gfx950): 4 wavefronts per SIMD by registers (64 of source + 16 sums), 17 KiB window + 16 KiB rings per workgroup.
#include <type_traits>

namespace pfv {

constexpr int kFsWaves = 4;                        // wavefronts per SIMD k_pf_search_full is compiled for
constexpr int kFsRingDwords = 16 * 64;             // per wavefront: 16 prefix sums per lane; first the macroblocks' source rows (8 x 256 B)
static_assert(kStripMB * 256 <= kFsRingDwords * 4, "the source hand-off fits the ring region");

// key of a candidate: E << 40 | (|dx| + |dy|) << 16 | (dy + 16) << 8 | (dx + 16); the minimum is the rule's choice
__device__ __forceinline__ unsigned long long fs_key(unsigned e, int dx, int dy)
{
    const unsigned lo = ((unsigned)(abs(dx) + abs(dy)) << 16) | ((unsigned)(dy + 16) << 8) | (unsigned)(dx + 16);
    return ((unsigned long long)e << 40) | lo;
}
// f(integral_constant<int, I>) for I = FIRST .. LAST - 1, unrolled
template <int FIRST, int LAST, class F>
__device__ __forceinline__ void fs_static_for(F &&f)
{
    if constexpr (FIRST < LAST) {
        f(std::integral_constant<int, FIRST>{});
        fs_static_for<FIRST + 1, LAST>(f);
    }
}
template <int CTRL>
__device__ __forceinline__ unsigned long long fs_min_step(unsigned long long v)
{
    const unsigned lo = (unsigned)dpp<CTRL>((int)(unsigned)v), hi = (unsigned)dpp<CTRL>((int)(unsigned)(v >> 32));
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o < v ? o : v;
}

__global__ __launch_bounds__(kThreads) PFV_WAVES_PER_EU(kFsWaves) void k_pf_search_full(FrameGeom g, const uint8_t *__restrict__ src,
                                                               const uint8_t *__restrict__ ref, int8_t *__restrict__ mv_out,
                                                               uint8_t *__restrict__ has_out, int16_t *__restrict__ coef,
                                                               uint8_t *__restrict__ recon, float min_err, int radius)
{
    __shared__ __attribute__((aligned(16))) uint8_t win_lds[16 + kWinAlloc];
    __shared__ __attribute__((aligned(16))) unsigned ring_lds[kStripsPerWG][kFsRingDwords];
    uint8_t *win = win_lds + 16;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = lane >> 3, i = lane & 7;
    const int vt = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const TilePos cur = locate_tile(g, vt, wave);
    const PlaneGeom &p = g.p[cur.sp.plane];
    issue_window(p, ref + (long)cur.sp.stream * g.pad_frame_bytes + p.pad_off, cur, win, wave, lane);
    uint4 rows[2];
    rows[0] = rows[1] = make_uint4(0, 0, 0, 0);
    if (cur.wave_valid) {
        const uint8_t *plane = frame_src(g, src, cur.sp.stream) + p.src_off;
        rows[0] = load_src16(plane, p, cur.sp.x0 + m * 16, cur.sp.y0 + i);
        rows[1] = load_src16(plane, p, cur.sp.x0 + m * 16, cur.sp.y0 + i + 8);
    }
    __syncthreads();   // window complete (vmcnt drained at the barrier); the only barrier of the kernel
    if (!cur.wave_valid) return;

    // all 16 source rows of the macroblock into every one of its lanes
    unsigned *ring = ring_lds[wave];
    uint4 a[16];
    {
        uint4 *blk = reinterpret_cast<uint4 *>(ring) + m * 16;
        blk[i] = rows[0];
        blk[i + 8] = rows[1];
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < 16; j++) a[j] = blk[j];
        wave_lds_sync();
    }
    unsigned s2 = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) s2 = sq4(rows[h].x, rows[h].y, rows[h].z, rows[h].w, s2);
    const unsigned a2 = (unsigned)mb_sum((int)s2);

    const int R = radius;
    const int mbx = cur.sp.x0 + m * 16, mby = cur.sp.y0;
    const int wcol0 = mbx - cur.winx0;             // = 16 + 16 m
    const int wrow0 = mby - cur.winy0;             // window row of source row 0: 15 + 16 wave
    unsigned long long best = ~0ull;
    for (int dx0 = -R; dx0 <= R; dx0 += 8) {       // wave-uniform trip count
        const int dx = dx0 + i;
        const int wx = wcol0 + min(dx, R), sh = wx & 3;      // a lane past the last column repeats column R; its keys are dropped
        const bool col_ok = dx <= R && mbx + dx >= 0 && mbx + dx <= p.pw - 16;
        const uint8_t *rp = win + (wrow0 - R) * kWinStride + (wx & ~3);
        unsigned acc[16];
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 0;
        unsigned prefix = 0;
        // Window row t of the column.  Chain slot j holds candidate t - j, which exists for 0 <= t - j <= 2R: slots JLO .. JHI take the row
        // (compile-time bounds: while the chain fills and drains, the products of candidates that do not exist are not issued), and with
        // EXIT slot 15 completes the candidate that started 15 rows above, dy = t - 15 - R.
        auto row = [&](auto jlo, auto jhi, auto exits, int t) {
            constexpr int JLO = decltype(jlo)::value, JHI = decltype(jhi)::value;
            const unsigned *d = reinterpret_cast<const unsigned *>(rp);
            const unsigned d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
            const unsigned b0 = __builtin_amdgcn_alignbyte(d1, d0, sh), b1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
            const unsigned b2 = __builtin_amdgcn_alignbyte(d3, d2, sh), b3 = __builtin_amdgcn_alignbyte(d4, d3, sh);
            if (decltype(exits)::value) {
                const unsigned before = ring[((t + 1) & 15) * 64 + lane];   // the prefix in front of row t - 15, left there 15 rows ago
                const unsigned ab = dot_ab(a[15], b0, b1, b2, b3, acc[14]);
                const unsigned bb = sq4(b0, b1, b2, b3, prefix) - before;
                const int dy = t - 15 - R;
                const unsigned e = a2 + bb - 2u * ab;
                const bool ok = col_ok && mby + dy >= 0 && mby + dy <= p.ph - 16;
                const unsigned long long key = ok ? fs_key(e, dx, dy) : ~0ull;
                best = key < best ? key : best;
            }
            ring[(t & 15) * 64 + lane] = prefix;    // what candidate dy = t - R does not contain
            prefix = sq4(b0, b1, b2, b3, prefix);
#pragma unroll
            for (int j = JHI; j >= JLO; j--) acc[j] = dot_ab(a[j], b0, b1, b2, b3, j ? acc[j ? j - 1 : 0] : 0u);
            rp += kWinStride;
        };
        using fs_false = std::integral_constant<bool, false>;
        using fs_true = std::integral_constant<bool, true>;
        // rows 0 .. 14: the chain fills, no candidate is complete (at R <= 7 the slots of rows past 2R carry candidates that do not
        // exist; the drain rows below never let them through)
        fs_static_for<0, 15>([&](auto t) { row(std::integral_constant<int, 0>{}, t, fs_false{}, decltype(t)::value); });
        // rows 15 .. 2R: every slot holds a candidate (no such row at R <= 7)
        for (int t = 15; t <= 2 * R; t++) row(std::integral_constant<int, 0>{}, std::integral_constant<int, 14>{}, fs_true{}, t);
        // rows 2R + k, k = 1 .. 15, from row 15 on: the chain drains, slots below k are empty
        fs_static_for<1, 16>([&](auto k) {
            if (2 * R + decltype(k)::value >= 15) row(k, std::integral_constant<int, 14>{}, fs_true{}, 2 * R + decltype(k)::value);
        });
    }
    best = fs_min_step<kQuadXor1>(best);
    best = fs_min_step<kQuadXor2>(best);
    best = fs_min_step<kRowHalfMirror>(best);
    // a macroblock slot past the strip's last macroblock has no candidate inside the plane (its key is still all ones): it fetches (0, 0)
    const bool mb_valid = m < cur.sp.n_mb;
    const int cx = mb_valid ? (int)((unsigned)best & 0xffu) - 16 : 0, cy = mb_valid ? (int)(((unsigned)best >> 8) & 0xffu) - 16 : 0;
    const unsigned err = (unsigned)(best >> 40);

    const bool coded = mb_valid && !((float)err <= min_err);   // skip decision (src/common.rs:209, :221)
    // the lane's two rows of the chosen patch (get_block of the reconstruction, :261)
    uint4 patch[2];
    {
        const int px = wcol0 + cx, shp = px & 3;
        const uint8_t *pp = win + (wrow0 + i + cy) * kWinStride + (px & ~3);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const unsigned *d = reinterpret_cast<const unsigned *>(pp + 8 * h * kWinStride);
            const unsigned d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
            patch[h] = make_uint4(__builtin_amdgcn_alignbyte(d1, d0, shp), __builtin_amdgcn_alignbyte(d2, d1, shp),
                                  __builtin_amdgcn_alignbyte(d3, d2, shp), __builtin_amdgcn_alignbyte(d4, d3, shp));
        }
    }
    if (mb_valid) {
        const long mbi = (long)cur.sp.stream * g.mbs_per_frame + cur.sp.mb_first + m;
        if (i == 0) {
            mv_out[mbi * 2 + 0] = (int8_t)cx;
            mv_out[mbi * 2 + 1] = (int8_t)cy;
            has_out[mbi] = coded ? 1 : 0;
        }
        if (!coded)
            penc_store_skipped(coef + mbi * 256, recon ? recon + (long)cur.sp.stream * g.pad_frame_bytes + p.pad_off + (long)(cur.sp.y0 + i) * p.pw + cur.sp.x0 + m * 16 : nullptr,
                               p.pw, i, patch);
    }
}

}  // namespace pfv
