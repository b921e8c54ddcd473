// pfv_scene_kernels.hip -- scene-cut measure on the device: what include/pfv_hip_ext.h defines ("scene-cut detection", normative).  Luma is
// reduced to quarter planes (k_scene_quarter), every 8 x 8 block of the current quarter plane is searched in the previous one within +-R
// quarter samples and measured against its own mean (k_scene_cost), and the block map is summed into one pfv_scene_stats per pair of frames
// (k_scene_sum).  Integer arithmetic only, no atomics, every output entry written by every run: the results do not depend on the launch shape.
// Included by pfv_capi.hip behind pfv_quality_kernels.hip (SseOperand, sse_load16, sse_mask); the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

#ifdef PFV_HIPEMU
// v_sad_u8 in plain C++: the emulator header has no such builtin
static inline unsigned scene_sad_u8(unsigned a, unsigned b, unsigned acc)
{
    for (int i = 0; i < 4; i++) {
        const int x = (int)((a >> (8 * i)) & 0xffu), y = (int)((b >> (8 * i)) & 0xffu);
        acc += (unsigned)(x > y ? x - y : y - x);
    }
    return acc;
}
#else
__device__ __forceinline__ unsigned scene_sad_u8(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }
#endif

constexpr int kSceneMaxR = 7;
constexpr int kSceneWinRows = 8 + 2 * kSceneMaxR;   // rows of the search window at the largest radius
constexpr int kSceneWinDw = 7;                      // dwords per window row: 8 + 2R samples from a 4-aligned column on, at most 3 + 22
constexpr unsigned kSceneNoCandidate = 0xffffffffu;

// Quarter planes of one launch group: qw x qh samples, rows qs bytes apart (a multiple of 8: a block's rows are aligned 8-byte loads), planes
// qbytes = qs * qh apart.  Samples at x >= qw inside a row are written as 0 and belong to no block and no candidate.
struct SceneGeom {
    int w, h;          // luma
    int qw, qh, qs;
    int nbx, nby;      // blocks of 8 x 8 quarter samples
    long qbytes;
};

// Frames -> quarter planes.  One lane per dword of a quarter row: 16 pixels of four source rows, loaded with k_sse_mb's front end (16-byte loads
// where legal, a byte path with the same result otherwise), the pixels beyond 4 qw masked, four v_dot4 per sample group.  n_frames x qh x qs / 4
// lanes; `src` is the frames' operand (its stream index is the frame of the launch).
__global__ __launch_bounds__(kThreads) void k_scene_quarter(SceneGeom sg, SseOperand src, int src_row, int n_frames, uint8_t *__restrict__ quarter)
{
    const int dpr = sg.qs >> 2;                       // dwords per quarter row
    const long per_frame = (long)sg.qh * dpr;
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= per_frame * n_frames) return;
    const int f = (int)(t / per_frame);
    const int rem = (int)(t - (long)f * per_frame);
    const int qy = rem / dpr, k = rem - qy * dpr;
    const uint8_t *plane = src.base + (long)f * src.stride;   // luma lies at offset 0 of either layout
    const bool vec = src.vec & 1;
    const int x = 16 * k, n = min(16, 4 * sg.qw - x);      // n: pixels of the segment that take part (<= 0: none)
    uint4 r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = sse_load16(src, plane, src_row, vec, x, 4 * qy + j, n, sg.h);   // 4 qy + 3 < h: the row test never fires
    unsigned out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned mk = sse_mask(n, i);
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned d = i == 0 ? r[j].x : (i == 1 ? r[j].y : (i == 2 ? r[j].z : r[j].w));
            s = __builtin_amdgcn_udot4(d & mk, 0x01010101u, s, false);
        }
        out |= ((s + 8u) >> 4) << (8 * i);            // at most (16 x 255 + 8) >> 4 = 255
    }
    *reinterpret_cast<unsigned *>(quarter + (long)f * sg.qbytes + (long)qy * sg.qs + 4 * k) = out;
}

// minimum over the wavefront, in every lane
__device__ __forceinline__ unsigned scene_wave_min(unsigned v)
{
    v = min(v, (unsigned)dpp<kQuadXor1>((int)v));
    v = min(v, (unsigned)dpp<kQuadXor2>((int)v));
    v = min(v, (unsigned)dpp<kRowHalfMirror>((int)v));
    v = min(v, (unsigned)dpp<0x140>((int)v));         // row_mirror: the other 8 lanes of the row
    v = min(v, (unsigned)__shfl_xor((int)v, 16));
    v = min(v, (unsigned)__shfl_xor((int)v, 32));
    return v;
}

// The previous quarter plane of pair p of a launch group.  run_dev (clip == 0): the state of stream `first + p` (`state` and `primed` point at the
// window's first stream).  run_clip_dev (clip != 0): the state of the one stream for p == 0, the quarter plane of frame p - 1 otherwise.
__device__ __forceinline__ const uint8_t *scene_prev(const SceneGeom &sg, const uint8_t *state, const uint8_t *quarter, const uint32_t *primed, int clip, int p,
                                                     bool &has_prev)
{
    if (clip && p > 0) {
        has_prev = true;
        return quarter + (long)(p - 1) * sg.qbytes;
    }
    has_prev = primed[clip ? 0 : p] != 0;
    return state + (clip ? 0 : (long)p * sg.qbytes);
}

// One wavefront per block.  The block's 16 dwords are wave-uniform loads; the (8 + 2R)^2 window of the previous plane is staged in LDS from a
// 4-aligned column on, as aligned dwords (a dword that does not lie inside the plane's rows reads as 0: no candidate that is allowed touches it).
// One lane per candidate, ceil((2R + 1)^2 / 64) passes: a candidate's row is three LDS dwords, two v_alignbyte, two v_sad_u8.  The tie rule is the
// minimum of one key, S << 12 | (|cx| + |cy|) << 8 | (cy + 7) << 4 | (cx + 7).
// blk: best << 16 | intra; vec: (cx, cy); aux (internal, for k_scene_sum): zero | moving << 16.  A pair without a previous frame writes zeros.
__global__ __launch_bounds__(kThreads) void k_scene_cost(SceneGeom sg, const uint8_t *__restrict__ state, const uint8_t *__restrict__ quarter,
                                                          const uint32_t *__restrict__ primed, int clip, int n_pairs, int R, uint32_t *__restrict__ blk,
                                                          int8_t *__restrict__ vec, uint32_t *__restrict__ aux)
{
    __shared__ unsigned win[kStripsPerWG][kSceneWinRows * kSceneWinDw];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_blocks = sg.nbx * sg.nby;
    const long gb = (long)blockIdx.x * kStripsPerWG + wave;
    if (gb >= (long)n_blocks * n_pairs) return;   // no cross-wavefront sync in this kernel
    const int p = (int)(gb / n_blocks), b = (int)(gb - (long)p * n_blocks);
    const int by = b / sg.nbx, bx = b - by * sg.nbx;
    bool has_prev;
    const uint8_t *prev = scene_prev(sg, state, quarter, primed, clip, p, has_prev);
    const long o = (long)p * n_blocks + b;
    if (!has_prev) {   // wave-uniform
        if (lane == 0) {
            blk[o] = 0;
            aux[o] = 0;
            vec[2 * o] = 0;
            vec[2 * o + 1] = 0;
        }
        return;
    }
    // the block
    const uint8_t *cur = quarter + (long)p * sg.qbytes + (long)(8 * by) * sg.qs + 8 * bx;
    unsigned c[16];
    unsigned sum = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint2 d = *reinterpret_cast<const uint2 *>(cur + (long)j * sg.qs);
        c[2 * j] = d.x;
        c[2 * j + 1] = d.y;
        sum = scene_sad_u8(d.y, 0u, scene_sad_u8(d.x, 0u, sum));
    }
    const unsigned mean4 = ((sum + 32u) >> 6) * 0x01010101u;
    unsigned intra = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) intra = scene_sad_u8(c[j], mean4, intra);
    // the window: rows 8 by - R .. 8 by + 7 + R, columns from ax = the 4-aligned column at or left of 8 bx - R
    const int rows = 8 + 2 * R, oy = 8 * by - R, ax = (8 * bx - R) & ~3;
    unsigned *w = win[wave];
    for (int i = lane; i < rows * kSceneWinDw; i += 64) {
        const int r = i / kSceneWinDw, k = i - r * kSceneWinDw;
        const int y = oy + r, x = ax + 4 * k;
        unsigned d = 0;
        if (y >= 0 && y < sg.qh && x >= 0 && x + 4 <= sg.qs) d = *reinterpret_cast<const unsigned *>(prev + (long)y * sg.qs + x);
        w[i] = d;
    }
    wave_lds_sync();
    const int side = 2 * R + 1, n_cand = side * side;
    const int zero_idx = R * side + R;                 // the candidate (0, 0): always allowed
    unsigned key = kSceneNoCandidate, zs = 0;
    for (int base = 0; base < n_cand; base += 64) {
        const int idx = base + lane;
        const int iy = idx / side, cy = iy - R, cx = idx - iy * side - R;
        const int px = 8 * bx + cx, py = 8 * by + cy;
        if (idx < n_cand && px >= 0 && px <= sg.qw - 8 && py >= 0 && py <= sg.qh - 8) {
            const int col = px - ax, dw = col >> 2, sh = col & 3;
            unsigned S = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const unsigned *row = w + (cy + R + j) * kSceneWinDw + dw;
                const unsigned d0 = row[0], d1 = row[1], d2 = row[2];
                S = scene_sad_u8(c[2 * j], __builtin_amdgcn_alignbyte(d1, d0, (unsigned)sh), S);
                S = scene_sad_u8(c[2 * j + 1], __builtin_amdgcn_alignbyte(d2, d1, (unsigned)sh), S);
            }
            const int ax_ = cx < 0 ? -cx : cx, ay_ = cy < 0 ? -cy : cy;
            key = min(key, (S << 12) | ((unsigned)(ax_ + ay_) << 8) | ((unsigned)(cy + 7) << 4) | (unsigned)(cx + 7));
            if (idx == zero_idx) zs = S;
        }
    }
    key = scene_wave_min(key);
    const unsigned zero = (unsigned)__shfl((int)zs, zero_idx & 63);
    if (lane == 0) {
        const unsigned best = key >> 12;
        const int cx = (int)(key & 15u) - 7, cy = (int)((key >> 4) & 15u) - 7;
        blk[o] = (best << 16) | intra;
        aux[o] = zero | ((cx != 0 || cy != 0) ? 0x10000u : 0u);
        vec[2 * o] = (int8_t)cx;
        vec[2 * o + 1] = (int8_t)cy;
    }
}

// a 64-bit sum over the wavefront, in every lane
__device__ __forceinline__ unsigned long long scene_wave_sum(unsigned long long acc)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)acc, off), hi = (unsigned)__shfl_xor((int)(unsigned)(acc >> 32), off);
        acc += ((unsigned long long)hi << 32) | lo;
    }
    return acc;
}

// The block map summed per pair, k_sse_sum's pattern: one workgroup per pair, every thread a strided share of the blocks, wave reduction, LDS,
// plain stores of the 40 bytes.  out: 10 dwords per pair (pfv_scene_stats: inter, intra, zero as 64-bit, n_blocks, n_intra, n_moving, reserved).
__global__ __launch_bounds__(kThreads) void k_scene_sum(SceneGeom sg, const uint32_t *__restrict__ blk, const uint32_t *__restrict__ aux,
                                                         const uint32_t *__restrict__ primed, int clip, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long part[kStripsPerWG][5];
    const int p = (int)blockIdx.x, n = sg.nbx * sg.nby;
    const bool has_prev = (clip && p > 0) || primed[clip ? 0 : p] != 0;
    unsigned long long inter = 0, intra = 0, zero = 0, n_intra = 0, n_moving = 0;
    if (has_prev)
        for (int k = threadIdx.x; k < n; k += kThreads) {
            const uint32_t v = blk[(long)p * n + k], a = aux[(long)p * n + k];
            inter += v >> 16;
            intra += v & 0xffffu;
            zero += a & 0xffffu;
            n_intra += (v >> 16) >= (v & 0xffffu) ? 1u : 0u;
            n_moving += a >> 16;
        }
    inter = scene_wave_sum(inter);
    intra = scene_wave_sum(intra);
    zero = scene_wave_sum(zero);
    n_intra = scene_wave_sum(n_intra);
    n_moving = scene_wave_sum(n_moving);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *q = part[threadIdx.x >> 6];
        q[0] = inter; q[1] = intra; q[2] = zero; q[3] = n_intra; q[4] = n_moving;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int wv = 0; wv < kStripsPerWG; wv++)
#pragma unroll
            for (int i = 0; i < 5; i++) tot[i] += part[wv][i];
        unsigned long long *dst = out + 5l * p;
        dst[0] = tot[0];
        dst[1] = tot[1];
        dst[2] = tot[2];
        dst[3] = (unsigned long long)(has_prev ? (unsigned)n : 0u) | (tot[3] << 32);   // n_blocks, n_intra (little-endian pair)
        dst[4] = tot[4];                                                               // n_moving, reserved = 0
    }
}

}  // namespace pfv
