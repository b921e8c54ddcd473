// pfv_prdprobe.hip -- the p-frame rate-distortion probe of an encoder session (pfv_enc_probe_pframe_rd*): payload bytes and squared error per
// plane of the window's frames as p-frames against the session's current prev_frame at every rung of the ladder, from one search and one forward
// transform.  Kernels: pfv_prdprobe_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip behind pfv_rdprobe.hip and pfv_pprobe.hip, never compiled on its own.

// the kernels' accumulators: the p-frame size probe's rows with min_err behind them (pprobe_acc) and the plane sums (rd_sums_acc)
static int prd_probe_acc(pfv_enc_session *s)
{
    pfv_ctx *ctx = s->ctx;
    if (ctx->capturing && (!s->pprobe_acc || !s->rd_acc))
        return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_pframe_rd_dev: the accumulator needs an allocation, which a graph recording cannot hold -- call once before pfv_graph_begin");
    int rc = pprobe_acc(s);
    if (!rc) rc = rd_sums_acc(s, "pfv_enc_probe_pframe_rd_dev");
    return rc;
}

static int prd_probe_launch(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev)
{
    pfv_ctx *ctx = s->ctx;
    int rc = prd_probe_acc(s);
    if (rc) return rc;
    const ProbeWin w = probe_win(s, frames_dev, true);
    const QTab *qt = (const QTab *)s->qtab_dev;
    uint32_t *acc = s->pprobe_acc + w.first * w.R * kPProbeAcc;
    unsigned long long *sse_acc = (unsigned long long *)s->rd_acc + w.first * w.R * 3;
    if (s->flt) hipLaunchKernelGGL(k_probe_pframe_rd<true>, dim3(penc_blocks(ctx, w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, w.ref, qt, s->n_rungs, w.min_err, -2, acc, sse_acc);
    else hipLaunchKernelGGL(k_probe_pframe_rd<false>, dim3(penc_blocks(ctx, w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, w.ref, qt, s->n_rungs, w.min_err, -2, acc, sse_acc);
    hipLaunchKernelGGL(k_pprobe_rd_sizes, dim3((unsigned)((size_t)s->win_count * w.R)), dim3(64), 0, ctx->stream, acc, sizes_dev + w.first * w.R,
                       stats_dev ? stats_dev + w.first * w.R * kPProbeStats : (uint32_t *)nullptr, sse_acc, (unsigned long long *)sse_dev + w.first * w.R * 3);
    return launch_check(ctx, "k_probe_pframe_rd / k_pprobe_rd_sizes");
}

// the frames in the session's staging (all slots, packed) -> sizes_out [n_streams][n_rungs], sse_out [n_streams][n_rungs][3] and, where asked
// for, stats_out [n_streams][n_rungs][kPProbeStats]: 28 bytes per (stream, rung), the counts behind them, through probe_download
static int prd_probe_staged(pfv_enc_session *s, uint32_t *sizes_out, uint64_t *sse_out, uint32_t *stats_out = nullptr)
{
    pfv_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->n_streams * (size_t)s->n_rungs;
    const size_t sse_bytes = n * 3 * sizeof(uint64_t), size_bytes = n * sizeof(uint32_t), stat_bytes = n * kPProbeStats * sizeof(uint32_t);
    if (!s->prd_out) HIP_TRY(ctx, hipMalloc((void **)&s->prd_out, sse_bytes + size_bytes + stat_bytes));
    uint32_t *sizes_dev = (uint32_t *)((uint8_t *)s->prd_out + sse_bytes);
    int rc = prd_probe_launch(s, s->st_frames, sizes_dev, s->prd_out, stats_out ? sizes_dev + n : nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return probe_download(ctx, s->prd_out, n, sse_out, nullptr, sizes_out, stats_out);
}

extern "C" {

PFV_API int pfv_enc_probe_pframe_rd_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev)
{
    if (int rf = enc_pframe_probe_refused(s, "pfv_enc_probe_pframe_rd_dev")) return rf;
    int rc = probe_dev_enter(s, frames_dev && sizes_dev && sse_dev, "pfv_enc_probe_pframe_rd_dev");
    return rc ? rc : prd_probe_launch(s, frames_dev, sizes_dev, sse_dev, stats_dev);
}
PFV_API int pfv_enc_probe_pframe_rd(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out)
{
    if (int rf = enc_pframe_probe_refused(s, "pfv_enc_probe_pframe_rd")) return rf;
    int rc = probe_host_enter(s, frames, sizes_out && sse_out, "pfv_enc_probe_pframe_rd");
    return rc ? rc : prd_probe_staged(s, sizes_out, sse_out);
}

}  // extern "C"
