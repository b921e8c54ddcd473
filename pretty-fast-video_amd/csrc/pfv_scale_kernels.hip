// pfv_scale_kernels.hip -- frame resize: n_streams planar Y | U | V 4:2:0 frames (packed or padded, where they lie) resampled to another size
// by a separable polyphase filter (k_scale).  Arithmetic: include/pfv_hip_ext.h, "frame resize" (normative): int16 coefficient rows that sum
// to 16384, a horizontal pass to 16-bit intermediates, a vertical pass to bytes, i32 throughout.  Both passes in one launch: the intermediate
// rows of a tile live in LDS only.  No atomics, no scratch, nothing in HBM between the passes.
// Included by pfv_capi.hip; the CPU emulator build compiles it unmodified.
#pragma once

namespace pfv {

constexpr int kScaleTW = 64, kScaleTH = 16;           // output tile of one workgroup: one lane per column, four rows per wavefront
constexpr int kScaleThreads = 256;
constexpr int kScaleMaxTaps = 48, kScaleMaxRatio = 8; // the ratio limit of the interface: n_src <= 8 * n_dst, so T <= 2 * ceil(3 * 8)
// first[] advances by at most ceil(ratio) per output, so a tile's taps span at most these many source rows / source bytes of a row
constexpr int kScaleRows = (kScaleTH - 1) * kScaleMaxRatio + kScaleMaxTaps;                  // 168
constexpr int kScaleRawDw = ((kScaleTW - 1) * kScaleMaxRatio + kScaleMaxTaps + 3 + 3) / 4 + 2;   // 140 dwords hold the span from its aligned start; 141: an odd pitch
constexpr int kScaleCxPitch = kScaleMaxTaps + 1;      // int16 coefficients of one column in s_cx: odd, so that neighbouring lanes' rows spread over the banks
constexpr int kScaleBatch = 8;                        // source rows staged per pass: 32 lanes per row; s_raw holds kScaleBatch rows of the widest span
constexpr int kScaleMaxBatch = 64;                    // rows per round where the span is narrow: a round is the rows that fit s_raw, in eights

struct ScaleAxis {
    const int32_t *first;    // [n_dst]
    const int16_t *coef;     // [n_dst][taps]
    int taps, n_src, n_dst;
};
struct ScalePlane {
    ScaleAxis x, y;
    long src_off, dst_off;   // byte offset of the plane inside one source / destination frame
    int src_pitch;           // bytes between source rows (the padded width for a padded source; indices are clamped to n_src all the same)
    int tiles_x, tile0;      // tiles per row of tiles; first tile of the plane inside one frame
};
struct ScaleArgs {
    ScalePlane p[3];
    const uint8_t *src;
    uint8_t *dst;
    long src_stride, dst_stride;   // bytes between the frames of consecutive streams
    int wide_src, wide_dst;        // bit p: plane p's rows may be read / written as aligned dwords
};

// Grid: x = the tiles of one frame (Y, then U, then V), y = the stream.  A workgroup
//   1. stages its columns' and its rows' first[] and coefficient rows in LDS (the rows are contiguous in memory: linear, coalesced copies),
//   2. per round of source rows (as many as fit s_raw, 8 .. 64): copies the byte span its columns' taps cover into LDS -- clamping to the PICTURE is done here, once
//      per byte: a dword that lies inside the picture of an aligned plane is one load, any other is put together from four clamped byte
//      loads -- and filters it horizontally into the 16-bit rows of s_t (two rows per lane and coefficient read),
//   3. filters vertically out of s_t (the output row, its first[] and coefficients are wave-uniform: LDS broadcasts), bytes into s_out,
//   4. stores s_out as dwords (non-temporal) where the plane's rows are aligned and the dword lies inside the tile, else byte by byte.
// LDS: 21 504 + 4 512 + 6 272 + 1 536 + 320 + 1 024 bytes.
__global__ __launch_bounds__(kScaleThreads) void k_scale(ScaleArgs a)
{
    __shared__ int16_t s_t[kScaleRows * kScaleTW];
    __shared__ unsigned s_raw[kScaleBatch * kScaleRawDw];
    __shared__ int16_t s_cx[kScaleTW * kScaleCxPitch];
    __shared__ int16_t s_cy[kScaleTH * kScaleMaxTaps];
    __shared__ int s_fx[kScaleTW], s_fy[kScaleTH];
    __shared__ unsigned s_out[kScaleTH * kScaleTW / 4];

    const int tid = (int)threadIdx.x;
    int tile = (int)blockIdx.x;
    const int pl = tile >= a.p[2].tile0 ? 2 : (tile >= a.p[1].tile0 ? 1 : 0);
    const ScalePlane &P = a.p[pl];
    tile -= P.tile0;
    const int tyi = tile / P.tiles_x, txi = tile - tyi * P.tiles_x;
    const int X0 = txi * kScaleTW, Y0 = tyi * kScaleTH;
    const int nX = min(kScaleTW, P.x.n_dst - X0), nY = min(kScaleTH, P.y.n_dst - Y0);
    const int Tx = P.x.taps, Ty = P.y.taps, sw = P.x.n_src, sh = P.y.n_src;      // both even: T = 2 * ceil(..) or 2 * S
    const int X = tid & 63, rs = __builtin_amdgcn_readfirstlane(tid >> 6), col = min(X, nX - 1);

    if (tid < kScaleTW) s_fx[tid] = P.x.first[X0 + min(tid, nX - 1)];
    else if (tid < kScaleTW + kScaleTH) s_fy[tid - kScaleTW] = P.y.first[Y0 + min(tid - kScaleTW, nY - 1)];
    {
        const int16_t *c = P.x.coef + (long)X0 * Tx;
        for (int i = tid; i < nX * Tx; i += kScaleThreads) {     // the tile's rows are contiguous: independent, coalesced loads
            const int c0 = i / Tx;
            s_cx[c0 * kScaleCxPitch + (i - c0 * Tx)] = c[i];
        }
        const int16_t *cy = P.y.coef + (long)Y0 * Ty;
        for (int i = tid; i < nY * Ty; i += kScaleThreads) s_cy[i] = cy[i];      // row yl's coefficients at s_cy[yl * Ty ..]
    }
    // the source span of the tile: bytes [ua4, ub] of rows [lo, hi]; ua4 and ub are not clamped (the staging clamps), lo and hi are
    const int ua4 = P.x.first[X0] & ~3, ub = P.x.first[X0 + nX - 1] + Tx - 1;
    const int ndw = min((ub - ua4) / 4 + 1, kScaleRawDw);
    const int pitch = ndw | 1;                                   // dwords between the staged rows: odd, at most kScaleRawDw
    const int batch = min((kScaleBatch * kScaleRawDw) / pitch, kScaleMaxBatch) & ~7;      // rows per round: 8 .. 64, a multiple of 8
    const int lo = min(max(P.y.first[Y0], 0), sh - 1), hi = min(max(P.y.first[Y0 + nY - 1] + Ty - 1, 0), sh - 1);
    const int nrows = min(hi - lo + 1, kScaleRows);
    const uint8_t *sp = a.src + (long)blockIdx.y * a.src_stride + P.src_off;
    const bool wide_src = (a.wide_src >> pl) & 1;
    __syncthreads();
    const int off = s_fx[col] - ua4;

    for (int r0 = 0; r0 < nrows; r0 += batch) {
        const int nb = min(batch, nrows - r0);
        for (int jb = tid >> 5; jb < nb; jb += 4 * kScaleBatch) {     // four passes of eight rows at a time: their loads are in flight together
            for (int d = tid & 31; d < ndw; d += 32) {
                const int x = ua4 + 4 * d;
                const bool one = wide_src && x >= 0 && x + 3 < sw;
                unsigned v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = jb + u * kScaleBatch;
                    v[u] = 0;
                    if (j < nb) {
                        const uint8_t *row = sp + (long)(lo + r0 + j) * P.src_pitch;
                        if (one) {
                            v[u] = *reinterpret_cast<const unsigned *>(row + x);
                        } else {
#pragma unroll
                            for (int b = 0; b < 4; b++) v[u] |= (unsigned)row[min(max(x + b, 0), sw - 1)] << (8 * b);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = jb + u * kScaleBatch;
                    if (j < nb) s_raw[j * pitch + d] = v[u];
                }
            }
        }
        __syncthreads();
        for (int j0 = rs; j0 < nb; j0 += 8) {                        // a wavefront filters rows j0 and j0 + 4 with one read of the coefficients
            const int j1 = j0 + 4 < nb ? j0 + 4 : j0;
            const uint8_t *b0 = reinterpret_cast<const uint8_t *>(s_raw + j0 * pitch) + off;
            const uint8_t *b1 = reinterpret_cast<const uint8_t *>(s_raw + j1 * pitch) + off;
            const int16_t *cx = s_cx + col * kScaleCxPitch;
            int acc0 = 0, acc1 = 0;
            for (int k = 0; k < Tx; k += 2) {                        // Tx is even: two taps per turn, their LDS reads in flight together
                const int c0 = cx[k], c1 = cx[k + 1];
                const int p00 = b0[k], p01 = b0[k + 1], p10 = b1[k], p11 = b1[k + 1];
                acc0 += c0 * p00 + c1 * p01;
                acc1 += c0 * p10 + c1 * p11;
            }
            s_t[(r0 + j0) * kScaleTW + X] = (int16_t)min(max((acc0 + 64) >> 7, -32768), 32767);
            s_t[(r0 + j1) * kScaleTW + X] = (int16_t)min(max((acc1 + 64) >> 7, -32768), 32767);
        }
        __syncthreads();
    }

    for (int yl = rs; yl < nY; yl += kScaleThreads / 64) {
        const int f = s_fy[yl];
        const int16_t *c = s_cy + yl * Ty;
        int acc = 0;
        for (int k = 0; k < Ty; k += 2) {                            // Ty is even
            const int ra = min(min(max(f + k, 0), sh - 1) - lo, kScaleRows - 1), rb = min(min(max(f + k + 1, 0), sh - 1) - lo, kScaleRows - 1);
            const int c0 = c[k], c1 = c[k + 1];
            const int t0 = s_t[ra * kScaleTW + X], t1 = s_t[rb * kScaleTW + X];
            acc += c0 * t0 + c1 * t1;
        }
        reinterpret_cast<uint8_t *>(s_out)[yl * kScaleTW + X] = (uint8_t)min(max((acc + (1 << 20)) >> 21, 0), 255);
    }
    __syncthreads();

    const int yl = tid >> 4, d = tid & 15;
    if (yl < nY && 4 * d < nX) {
        uint8_t *o = a.dst + (long)blockIdx.y * a.dst_stride + P.dst_off + (long)(Y0 + yl) * P.x.n_dst + X0 + 4 * d;
        const unsigned v = s_out[yl * (kScaleTW / 4) + d];
        if (((a.wide_dst >> pl) & 1) && 4 * d + 3 < nX) {
            __builtin_nontemporal_store(v, reinterpret_cast<unsigned *>(o));
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (4 * d + b < nX) o[b] = (uint8_t)(v >> (8 * b));
        }
    }
}

}  // namespace pfv
