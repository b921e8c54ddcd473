// pfv_ssimprobe.hip -- the SSIM probe of an encoder session (pfv_enc_probe_iframe_ssim*, pfv_enc_probe_pframe_ssim*): payload bytes, squared
// error per plane and the SSIM sums per plane of the window's frames as i-frames, or as p-frames against the session's current prev_frame, at
// every rung of the ladder.  Kernels: pfv_ssimprobe_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip behind pfv_prdprobe.hip, never compiled on its own.

// the block-sum map of the session, n_streams * mbs_per_frame * (n_rungs * 128 + 64) bytes: made by the first call, never cleared (every
// call writes all of its window's part before it reads it), freed with the session
static int ssim_probe_map(pfv_enc_session *s, bool pframe, const char *who)
{
    pfv_ctx *ctx = s->ctx;
    const bool have = s->ssim_probe_map && (pframe ? s->pprobe_acc : s->probe_acc) && s->rd_acc;
    if (ctx->capturing && !have)
        return fail(ctx, PFV_ERR_STATE, std::string(who) + ": the block-sum map and the accumulators need an allocation, which a graph recording cannot hold -- call once before pfv_graph_begin");
    int rc = pframe ? pprobe_acc(s) : probe_acc(s);
    if (!rc) rc = rd_sums_acc(s, who);
    if (rc || s->ssim_probe_map) return rc;
    HIP_TRY(ctx, hipMalloc((void **)&s->ssim_probe_map, (size_t)s->n_streams * ssim_map_stream_dwords(s->geom.mbs_per_frame, s->n_rungs) * sizeof(uint32_t)));
    return PFV_OK;
}

// the probe kernel, the windows, the RD probes' tail
static int ssim_probe_launch(pfv_enc_session *s, bool pframe, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, int64_t *ssim_dev, uint32_t *stats_dev)
{
    pfv_ctx *ctx = s->ctx;
    int rc = ssim_probe_map(s, pframe, pframe ? "pfv_enc_probe_pframe_ssim_dev" : "pfv_enc_probe_iframe_ssim_dev");
    if (rc) return rc;
    const ProbeWin w = probe_win(s, frames_dev, pframe);
    const QTab *qt = (const QTab *)s->qtab_dev;
    unsigned long long *sse_acc = (unsigned long long *)s->rd_acc + w.first * w.R * 3, *sse_out = (unsigned long long *)sse_dev + w.first * w.R * 3;
    uint32_t *map = s->ssim_probe_map + w.first * ssim_map_stream_dwords(w.g.mbs_per_frame, s->n_rungs);
    uint32_t *acc = pframe ? s->pprobe_acc + w.first * w.R * kPProbeAcc : s->probe_acc + w.first * w.R * kProbeAcc;
    const unsigned rows = (unsigned)((size_t)s->win_count * w.R);
    if (pframe) {
        if (s->flt) hipLaunchKernelGGL(k_probe_pframe_ssim<true>, dim3(penc_blocks(ctx, w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, w.ref, qt, s->n_rungs, w.min_err, -2, acc, sse_acc, map);
        else hipLaunchKernelGGL(k_probe_pframe_ssim<false>, dim3(penc_blocks(ctx, w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, w.ref, qt, s->n_rungs, w.min_err, -2, acc, sse_acc, map);
    } else if (use_small_grid(s->lane_mapping, w.g)) {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe_ssim<true, 16>), dim3(half_strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc, map);
        else hipLaunchKernelGGL((k_probe_iframe_ssim<false, 16>), dim3(half_strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc, map);
    } else {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe_ssim<true, 8>), dim3(strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc, map);
        else hipLaunchKernelGGL((k_probe_iframe_ssim<false, 8>), dim3(strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc, map);
    }
    hipLaunchKernelGGL(k_probe_ssim_windows, dim3(rows), dim3(kThreads), 0, ctx->stream, w.g, s->n_rungs, (const uint32_t *)map, ssim_dev + w.first * w.R * 3);
    if (pframe)
        hipLaunchKernelGGL(k_pprobe_rd_sizes, dim3(rows), dim3(64), 0, ctx->stream, acc, sizes_dev + w.first * w.R,
                           stats_dev ? stats_dev + w.first * w.R * kPProbeStats : (uint32_t *)nullptr, sse_acc, sse_out);
    else
        hipLaunchKernelGGL(k_probe_rd_sizes, dim3(rows), dim3(64), 0, ctx->stream, acc, sizes_dev + w.first * w.R,
                           stats_dev ? stats_dev + w.first * w.R * kProbeStats : (uint32_t *)nullptr, sse_acc, sse_out);
    return launch_check(ctx, pframe ? "k_probe_pframe_ssim / k_probe_ssim_windows / k_pprobe_rd_sizes" : "k_probe_iframe_ssim / k_probe_ssim_windows / k_probe_rd_sizes");
}

// the frames in the session's staging (all slots, packed) -> sizes_out [n_streams][n_rungs], sse_out and ssim_out [n_streams][n_rungs][3] and,
// where asked for (p-frames), counts_out [n_streams][n_rungs][kPProbeStats]: 52 bytes per (stream, rung), the counts behind them, through
// probe_download
static int ssim_probe_staged(pfv_enc_session *s, bool pframe, uint32_t *sizes_out, uint64_t *sse_out, int64_t *ssim_out, uint32_t *counts_out = nullptr)
{
    pfv_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->n_streams * (size_t)s->n_rungs;
    const size_t sum_bytes = n * 3 * sizeof(uint64_t), size_bytes = n * sizeof(uint32_t), stat_bytes = n * kPProbeStats * sizeof(uint32_t);
    if (!s->ssim_probe_out) HIP_TRY(ctx, hipMalloc((void **)&s->ssim_probe_out, 2 * sum_bytes + size_bytes + stat_bytes));
    uint8_t *out = (uint8_t *)s->ssim_probe_out;
    uint32_t *sizes_dev = (uint32_t *)(out + 2 * sum_bytes);
    int rc = ssim_probe_launch(s, pframe, s->st_frames, sizes_dev, (uint64_t *)out, (int64_t *)(out + sum_bytes), counts_out ? sizes_dev + n : nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return probe_download(ctx, out, n, sse_out, ssim_out, sizes_out, counts_out);
}

extern "C" {

PFV_API int pfv_enc_probe_iframe_ssim_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, int64_t *ssim_q24_dev, uint32_t *stats_dev)
{
    int rc = probe_dev_enter(s, frames_dev && sizes_dev && sse_dev && ssim_q24_dev, "pfv_enc_probe_iframe_ssim_dev");
    return rc ? rc : ssim_probe_launch(s, false, frames_dev, sizes_dev, sse_dev, ssim_q24_dev, stats_dev);
}
PFV_API int pfv_enc_probe_iframe_ssim(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out, int64_t *ssim_q24_out)
{
    int rc = probe_host_enter(s, frames, sizes_out && sse_out && ssim_q24_out, "pfv_enc_probe_iframe_ssim");
    return rc ? rc : ssim_probe_staged(s, false, sizes_out, sse_out, ssim_q24_out);
}
PFV_API int pfv_enc_probe_pframe_ssim_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, int64_t *ssim_q24_dev, uint32_t *stats_dev)
{
    if (int rf = enc_pframe_probe_refused(s, "pfv_enc_probe_pframe_ssim_dev")) return rf;
    int rc = probe_dev_enter(s, frames_dev && sizes_dev && sse_dev && ssim_q24_dev, "pfv_enc_probe_pframe_ssim_dev");
    return rc ? rc : ssim_probe_launch(s, true, frames_dev, sizes_dev, sse_dev, ssim_q24_dev, stats_dev);
}
PFV_API int pfv_enc_probe_pframe_ssim(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out, int64_t *ssim_q24_out)
{
    if (int rf = enc_pframe_probe_refused(s, "pfv_enc_probe_pframe_ssim")) return rf;
    int rc = probe_host_enter(s, frames, sizes_out && sse_out && ssim_q24_out, "pfv_enc_probe_pframe_ssim");
    return rc ? rc : ssim_probe_staged(s, true, sizes_out, sse_out, ssim_q24_out);
}

}  // extern "C"
