// pfv_hiersearch_kernels.hip -- k_halve, k_pf_search_coarse, k_pf_refine: two-level motion search of a p-frame (PFV_SEARCH_HIER,
// include/pfv_hip_ext.h).  Included by pfv_capi.hip behind pfv_fullsearch_kernels.hip, whose key minimum and unrolling helpers it uses.
//
// Four launches in front of k_pf_transform:
//   k_halve<false>       the launch's source frames (frame_src: stride or slot table, clear-fill pad) -> half planes, 2 x 2 rounded mean;
//   k_halve<true>        the padded reference -> half planes;
//   k_pf_search_coarse   every (cx, cy) with |cx|, |cy| <= Rc on the half planes, 8 x 8 blocks -> one coarse vector per macroblock;
//   k_pf_refine          (0, 0) and the 25 full-resolution vectors round twice the coarse one -> mv, flag, a skipped macroblock finished.
//
// Half planes: pw/2 x ph/2 pixels at a row pitch of (pw/2 rounded up to 16) bytes, the three planes of a slot back to back, slots
// HalfGeom::frame_bytes apart.  Pitch and offsets are multiples of 16, so the coarse window is staged by the 16-byte global->LDS DMA of
// issue_window with the same out-of-plane redirect, also for the 8-pixel-wide half of a 16 x 16 plane.
//
// k_pf_search_coarse is k_pf_search_full at half size.  A 128 x 64 tile is 64 x 32 there and its +-31 window 126 bytes x 94 rows: the
// window buffer of k_pf_search (kWinRows x kWinStride) with the origin at (x0/2 - 32, y0/2 - 31).  Lane (m, i) owns the columns
// cx = -Rc + i + 8k of macroblock m and keeps the block's 8 source rows in 16 registers; a window row is read (3 aligned dwords), shifted
// (2 v_alignbyte) and squared (2 v_dot4) once and feeds 8 running sums on a v_dot4 accumulator chain; sum b^2 of a candidate is the difference
// of two prefix sums, the older one out of an 8-entry ring in LDS (lane-linear).  The rows in which the chain fills and drains are unrolled.
// E = sum a^2 - 2 sum ab + sum b^2 is exact in u32 (< 2^22).  One 64-bit DPP minimum per macroblock.
//
// k_pf_refine has no tile window: neighbouring macroblocks look at different places.  Lane (m, i) keeps source rows i and i + 8 and reads
// the two rows of every candidate from the reference plane as unaligned 16-byte loads (L2-resident); the macroblock's 8 partial sums meet
// in mb_sum.  One wavefront per strip.
namespace pfv {

constexpr int kHsWaves = 6;                        // wavefronts per SIMD k_pf_search_coarse is compiled for
constexpr int kHsRingDwords = 8 * 64;              // per wavefront: 8 prefix sums per lane
constexpr int kHsReach = 31;                       // largest Rc: the window's margin
static_assert(16 * kStripsPerWG / 2 + 2 * kHsReach <= kWinRows && 8 * kStripMB + 2 * kHsReach + 2 <= kWinStride - 16, "the half-resolution window fits k_pf_search's");

// where the half planes of a slot lie (host: half_geom in pfv_launch.hip)
struct HalfGeom {
    int pitch[3];        // bytes per row: pw / 2 rounded up to 16
    long off[3];         // byte offset of the plane inside one half frame
    long frame_bytes;    // stride between slots
};

// key of a coarse candidate: E << 40 | (|cx| + |cy|) << 16 | (cy + 32) << 8 | (cx + 32)
__device__ __forceinline__ unsigned long long hs_key(unsigned e, int cx, int cy)
{
    const unsigned lo = ((unsigned)(abs(cx) + abs(cy)) << 16) | ((unsigned)(cy + 32) << 8) | (unsigned)(cx + 32);
    return ((unsigned long long)e << 40) | lo;
}
// key of a fine candidate: the same with a bias of 64
__device__ __forceinline__ unsigned long long hr_key(unsigned e, int dx, int dy)
{
    const unsigned lo = ((unsigned)(abs(dx) + abs(dy)) << 16) | ((unsigned)(dy + 64) << 8) | (unsigned)(dx + 64);
    return ((unsigned long long)e << 40) | lo;
}

// four pixels of the 2 x 2 rounded mean from 8 pixels of two rows: the byte pairs are added as 16-bit fields
__device__ __forceinline__ unsigned halve4(const uint2 &r0, const uint2 &r1)
{
    const unsigned k = 0x00ff00ffu;
    const unsigned sx = ((((r0.x & k) + ((r0.x >> 8) & k) + (r1.x & k) + ((r1.x >> 8) & k) + 0x00020002u) >> 2) & k);
    const unsigned sy = ((((r0.y & k) + ((r0.y >> 8) & k) + (r1.y & k) + ((r1.y >> 8) & k) + 0x00020002u) >> 2) & k);
    return (sx & 0xffu) | ((sx >> 16) << 8) | ((sy & 0xffu) << 16) | ((sy >> 16) << 24);
}
// 8 source pixels (x .. x + 7, row y) of an unpadded plane with load_src16's pad rule; x is a multiple of 8
__device__ __forceinline__ uint2 load_src8(const uint8_t *plane, const PlaneGeom &p, int x, int y)
{
    const unsigned fill = (unsigned)p.clear * 0x01010101u;
    uint2 val = make_uint2(fill, fill);
    if (y < p.h && x < p.w) {
        const uint8_t *src = plane + (long)y * p.w + x;
        if (p.fast_src && x + 8 <= p.w) {
            val = *reinterpret_cast<const uint2 *>(src);
        } else {
            unsigned wds[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                unsigned acc = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int xx = x + i * 4 + b;
                    const unsigned px = xx < p.w ? (unsigned)src[i * 4 + b] : (unsigned)p.clear;
                    acc |= px << (8 * b);
                }
                wds[i] = acc;
            }
            val = make_uint2(wds[0], wds[1]);
        }
    }
    return val;
}

// One thread per dword of the half frames of all slots.  PADDED: `in` is a padded frame array (the reference); otherwise the launch's source
// frames.  The bytes between pw / 2 and the pitch are written as zero and never read as pixels.
template <bool PADDED>
__global__ __launch_bounds__(kThreads) void k_halve(FrameGeom g, HalfGeom hg, const uint8_t *__restrict__ in, uint8_t *__restrict__ out)
{
    const long per_frame = hg.frame_bytes >> 2;
    const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= per_frame * g.n_streams) return;
    const int stream = (int)(idx / per_frame);
    long b = (idx - (long)stream * per_frame) * 4;
    const int plane = (g.n_planes > 2 && b >= hg.off[2]) ? 2 : ((g.n_planes > 1 && b >= hg.off[1]) ? 1 : 0);
    const PlaneGeom &p = g.p[plane];
    b -= hg.off[plane];
    const int y = (int)(b / hg.pitch[plane]), x = (int)(b - (long)y * hg.pitch[plane]);
    unsigned val = 0;
    if (x < (p.pw >> 1)) {
        uint2 r0, r1;
        if (PADDED) {
            const uint8_t *row = in + (long)stream * g.pad_frame_bytes + p.pad_off + (long)(2 * y) * p.pw + 2 * x;
            r0 = *reinterpret_cast<const uint2 *>(row);
            r1 = *reinterpret_cast<const uint2 *>(row + p.pw);
        } else {
            const uint8_t *pl = frame_src(g, in, stream) + p.src_off;
            r0 = load_src8(pl, p, 2 * x, 2 * y);
            r1 = load_src8(pl, p, 2 * x, 2 * y + 1);
        }
        val = halve4(r0, r1);
    }
    *reinterpret_cast<unsigned *>(out + (long)stream * hg.frame_bytes + hg.off[plane] + b) = val;
}

// sum a.b over one 8-pixel row
__device__ __forceinline__ unsigned dot_ab8(const uint2 &a, unsigned b0, unsigned b1, unsigned acc)
{
    return __builtin_amdgcn_udot4(a.y, b1, __builtin_amdgcn_udot4(a.x, b0, acc, false), false);
}

__global__ __launch_bounds__(kThreads) PFV_WAVES_PER_EU(kHsWaves) void k_pf_search_coarse(FrameGeom g, HalfGeom hg, const uint8_t *__restrict__ hsrc,
                                                                 const uint8_t *__restrict__ href, int8_t *__restrict__ cmv_out, int rc)
{
    __shared__ __attribute__((aligned(16))) uint8_t win_lds[16 + kWinAlloc];
    __shared__ __attribute__((aligned(16))) unsigned ring_lds[kStripsPerWG][kHsRingDwords];
    uint8_t *win = win_lds + 16;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = lane >> 3, i = lane & 7;
    const int vt = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const TilePos cur = locate_tile(g, vt, wave);
    const PlaneGeom &p = g.p[cur.sp.plane];
    const int pitch = hg.pitch[cur.sp.plane], hpw = p.pw >> 1, hph = p.ph >> 1;
    const long hbase = (long)cur.sp.stream * hg.frame_bytes + hg.off[cur.sp.plane];
    const int winx0 = (cur.sp.x0 >> 1) - 32, winy0 = cur.plane_ty * (8 * kStripsPerWG) - kHsReach;
    {   // issue_window on the half plane: chunks outside it are redirected to a clamped address inside, their content is never used
        const uint8_t *refp = href + hbase;
        const int q0 = win_first_issue(wave), q1 = win_first_issue(wave + 1);
#pragma unroll 5
        for (int q = q0; q < q1; q++) {
            const int c = q * 64 + lane;
            const int row = c / kWinChunksPerRow, col = c - row * kWinChunksPerRow;
            const int y = min(max(winy0 + row, 0), hph - 1), x = min(max(winx0 + col * 16, 0), pitch - 16);
            __builtin_amdgcn_global_load_lds((gbl_cvoid_t *)(refp + (long)y * pitch + x), (lds_void_t *)(win + c * 16), 16, 0, 0);
        }
    }
    const bool mb_valid = cur.wave_valid && m < cur.sp.n_mb;
    const int hbx = (cur.sp.x0 >> 1) + m * 8, hby = cur.sp.y0 >> 1;
    uint2 a[8];
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = make_uint2(0, 0);
    if (mb_valid) {
        const uint8_t *sp = hsrc + hbase + (long)hby * pitch + hbx;
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] = *reinterpret_cast<const uint2 *>(sp + (long)j * pitch);
    }
    __syncthreads();   // window complete (vmcnt drained at the barrier); the only barrier of the kernel
    if (!cur.wave_valid) return;

    unsigned *ring = ring_lds[wave];
    unsigned a2 = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) a2 = sq2(a[j].x, a[j].y, a2);

    const int R = rc;
    const int wcol0 = hbx - winx0;                 // = 32 + 8 m
    const int wrow0 = hby - winy0;                 // window row of source row 0: 31 + 8 wave
    unsigned long long best = ~0ull;
    for (int dx0 = -R; dx0 <= R; dx0 += 8) {       // wave-uniform trip count
        const int dx = dx0 + i;
        const int wx = wcol0 + min(dx, R), sh = wx & 3;      // a lane past the last column repeats column R; its keys are dropped
        const bool col_ok = dx <= R && hbx + dx >= 0 && hbx + dx <= hpw - 8;
        const uint8_t *rp = win + (wrow0 - R) * kWinStride + (wx & ~3);
        unsigned acc[8];
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] = 0;
        unsigned prefix = 0;
        // Window row t of the column.  Chain slot j holds candidate t - j, which exists for 0 <= t - j <= 2R: slots JLO .. JHI take the row,
        // and with EXIT slot 7 completes the candidate that started 7 rows above, cy = t - 7 - R (k_pf_search_full's scheme at 8 rows).
        auto row = [&](auto jlo, auto jhi, auto exits, int t) {
            constexpr int JLO = decltype(jlo)::value, JHI = decltype(jhi)::value;
            const unsigned *d = reinterpret_cast<const unsigned *>(rp);
            const unsigned d0 = d[0], d1 = d[1], d2 = d[2];
            const unsigned b0 = __builtin_amdgcn_alignbyte(d1, d0, sh), b1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
            if (decltype(exits)::value) {
                const unsigned before = ring[((t + 1) & 7) * 64 + lane];   // the prefix in front of row t - 7, left there 7 rows ago
                const unsigned ab = dot_ab8(a[7], b0, b1, acc[6]);
                const unsigned bb = sq2(b0, b1, prefix) - before;
                const int dy = t - 7 - R;
                const unsigned e = a2 + bb - 2u * ab;
                const bool ok = col_ok && hby + dy >= 0 && hby + dy <= hph - 8;
                const unsigned long long key = ok ? hs_key(e, dx, dy) : ~0ull;
                best = key < best ? key : best;
            }
            ring[(t & 7) * 64 + lane] = prefix;     // what candidate cy = t - R does not contain
            prefix = sq2(b0, b1, prefix);
#pragma unroll
            for (int j = JHI; j >= JLO; j--) acc[j] = dot_ab8(a[j], b0, b1, j ? acc[j ? j - 1 : 0] : 0u);
            rp += kWinStride;
        };
        using hs_false = std::integral_constant<bool, false>;
        using hs_true = std::integral_constant<bool, true>;
        // rows 0 .. 6: the chain fills, no candidate is complete (at Rc <= 3 the slots of rows past 2R carry candidates that do not exist;
        // the drain rows below never let them through)
        fs_static_for<0, 7>([&](auto t) { row(std::integral_constant<int, 0>{}, t, hs_false{}, decltype(t)::value); });
        // rows 7 .. 2R: every slot holds a candidate (no such row at Rc <= 3)
        for (int t = 7; t <= 2 * R; t++) row(std::integral_constant<int, 0>{}, std::integral_constant<int, 6>{}, hs_true{}, t);
        // rows 2R + k, k = 1 .. 7, from row 7 on: the chain drains, slots below k are empty
        fs_static_for<1, 8>([&](auto k) {
            if (2 * R + decltype(k)::value >= 7) row(k, std::integral_constant<int, 6>{}, hs_true{}, 2 * R + decltype(k)::value);
        });
    }
    best = fs_min_step<kQuadXor1>(best);
    best = fs_min_step<kQuadXor2>(best);
    best = fs_min_step<kRowHalfMirror>(best);
    if (mb_valid && i == 0) {
        const long mbi = (long)cur.sp.stream * g.mbs_per_frame + cur.sp.mb_first + m;
        cmv_out[mbi * 2 + 0] = (int8_t)((int)((unsigned)best & 0xffu) - 32);
        cmv_out[mbi * 2 + 1] = (int8_t)((int)(((unsigned)best >> 8) & 0xffu) - 32);
    }
}

constexpr int kHrWaves = 8;   // wavefronts per SIMD k_pf_refine is compiled for: no LDS, latency-bound on the reference rows
__global__ __launch_bounds__(kThreads) PFV_WAVES_PER_EU(kHrWaves) void k_pf_refine(FrameGeom g, const uint8_t *__restrict__ src, const uint8_t *__restrict__ ref,
                                                          const int8_t *__restrict__ cmv, int8_t *__restrict__ mv_out, uint8_t *__restrict__ has_out,
                                                          int16_t *__restrict__ coef, uint8_t *__restrict__ recon, float min_err)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = lane >> 3, i = lane & 7;
    const int gstrip = (int)blockIdx.x * kStripsPerWG + wave;
    if (gstrip >= g.strips_per_frame * g.n_streams) return;
    const StripPos sp = locate_strip(g, gstrip);
    const PlaneGeom &p = g.p[sp.plane];
    const bool mb_valid = m < sp.n_mb;
    const int mbx = sp.x0 + (mb_valid ? m : 0) * 16, mby = sp.y0;      // a slot past the strip's last macroblock reads macroblock 0's rows
    const long mbi = (long)sp.stream * g.mbs_per_frame + sp.mb_first + (mb_valid ? m : 0);
    const uint8_t *plane = frame_src(g, src, sp.stream) + p.src_off;
    const uint4 a0 = load_src16(plane, p, mbx, mby + i), a1 = load_src16(plane, p, mbx, mby + i + 8);
    const int c2x = 2 * (int)cmv[mbi * 2 + 0], c2y = 2 * (int)cmv[mbi * 2 + 1];
    const unsigned a2 = sq4(a1.x, a1.y, a1.z, a1.w, sq4(a0.x, a0.y, a0.z, a0.w, 0u));
    const uint8_t *rrow = ref + (long)sp.stream * g.pad_frame_bytes + p.pad_off + (long)(mby + i) * p.pw + mbx;
    unsigned long long best = ~0ull;
#pragma unroll 2
    for (int c = 0; c < 26; c++) {                                     // 25 round twice the coarse vector, then (0, 0)
        const int ry = c / 5, rx = c - ry * 5;
        const int dx = c < 25 ? c2x + rx - 2 : 0, dy = c < 25 ? c2y + ry - 2 : 0;
        const bool ok = abs(dx) <= 63 && abs(dy) <= 63 && mbx + dx >= 0 && mbx + dx <= p.pw - 16 && mby + dy >= 0 && mby + dy <= p.ph - 16;
        const uint8_t *bp = rrow + (ok ? (long)dy * p.pw + dx : 0);    // a candidate outside the plane reads (0, 0); its key is dropped
        const uint4 b0 = load_unaligned16(bp), b1 = load_unaligned16(bp + 8 * (long)p.pw);
        const unsigned bb = sq4(b1.x, b1.y, b1.z, b1.w, sq4(b0.x, b0.y, b0.z, b0.w, 0u));
        const unsigned ab = dot_ab(a1, b1.x, b1.y, b1.z, b1.w, dot_ab(a0, b0.x, b0.y, b0.z, b0.w, 0u));
        const unsigned e = (unsigned)mb_sum((int)(a2 + bb - 2u * ab));   // the lanes' parts wrap, their sum is exact (< 2^24)
        const unsigned long long key = ok ? hr_key(e, dx, dy) : ~0ull;
        best = key < best ? key : best;
    }
    const int cx = (int)((unsigned)best & 0xffu) - 64, cy = (int)(((unsigned)best >> 8) & 0xffu) - 64;
    const unsigned err = (unsigned)(best >> 40);
    const bool coded = !((float)err <= min_err);   // skip decision (src/common.rs:209, :221)
    if (mb_valid) {
        if (i == 0) {
            mv_out[mbi * 2 + 0] = (int8_t)cx;
            mv_out[mbi * 2 + 1] = (int8_t)cy;
            has_out[mbi] = coded ? 1 : 0;
        }
        if (!coded) {
            const uint8_t *pp = rrow + (long)cy * p.pw + cx;
            uint4 patch[2];
            patch[0] = load_unaligned16(pp);
            patch[1] = load_unaligned16(pp + 8 * (long)p.pw);
            penc_store_skipped(coef + mbi * 256, recon ? recon + (long)sp.stream * g.pad_frame_bytes + p.pad_off + (long)(mby + i) * p.pw + mbx : nullptr, p.pw, i, patch);
        }
    }
}

}  // namespace pfv
