// pfv_rdprobe.hip -- the i-frame rate-distortion probe of an encoder session (pfv_enc_probe_iframe_rd*): payload bytes and squared error per
// plane of the window's frames as i-frames at every rung of the ladder, from one read of the frames.  Kernels: pfv_rdprobe_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip behind pfv_probe.hip, never compiled on its own.

// the plane sums' accumulator [n_streams][n_rungs][3], shared by both rate-distortion probes (calls are ordered on the context's stream): made and
// cleared by the first call, left clear by every k_probe_rd_sizes / k_pprobe_rd_sizes
static int rd_sums_acc(pfv_enc_session *s, const char *who)
{
    pfv_ctx *ctx = s->ctx;
    if (s->rd_acc) return PFV_OK;
    const size_t bytes = (size_t)s->n_streams * (size_t)s->n_rungs * 3 * sizeof(uint64_t);
    HIP_TRY(ctx, hipMalloc((void **)&s->rd_acc, bytes));
    hipError_t e = hipMemsetAsync(s->rd_acc, 0, bytes, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(s->rd_acc);
        s->rd_acc = nullptr;
        return hip_fail(ctx, e, who);
    }
    return PFV_OK;
}
// the kernels' accumulators: the size probe's rows (probe_acc) and the plane sums
static int rd_probe_acc(pfv_enc_session *s)
{
    pfv_ctx *ctx = s->ctx;
    if (ctx->capturing && (!s->probe_acc || !s->rd_acc))
        return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_iframe_rd_dev: the accumulator needs an allocation, which a graph recording cannot hold -- call once before pfv_graph_begin");
    int rc = probe_acc(s);
    if (!rc) rc = rd_sums_acc(s, "pfv_enc_probe_iframe_rd_dev");
    return rc;
}

static int rd_probe_launch(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev)
{
    pfv_ctx *ctx = s->ctx;
    int rc = rd_probe_acc(s);
    if (rc) return rc;
    const ProbeWin w = probe_win(s, frames_dev, false);
    const QTab *qt = (const QTab *)s->qtab_dev;
    uint32_t *acc = s->probe_acc + w.first * w.R * kProbeAcc;
    unsigned long long *sse_acc = (unsigned long long *)s->rd_acc + w.first * w.R * 3;
    if (use_small_grid(s->lane_mapping, w.g)) {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe_rd<true, 16>), dim3(half_strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc);
        else hipLaunchKernelGGL((k_probe_iframe_rd<false, 16>), dim3(half_strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc);
    } else {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe_rd<true, 8>), dim3(strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc);
        else hipLaunchKernelGGL((k_probe_iframe_rd<false, 8>), dim3(strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc, sse_acc);
    }
    hipLaunchKernelGGL(k_probe_rd_sizes, dim3((unsigned)((size_t)s->win_count * w.R)), dim3(64), 0, ctx->stream, acc, sizes_dev + w.first * w.R,
                       stats_dev ? stats_dev + w.first * w.R * kProbeStats : (uint32_t *)nullptr, sse_acc, (unsigned long long *)sse_dev + w.first * w.R * 3);
    return launch_check(ctx, "k_probe_iframe_rd / k_probe_rd_sizes");
}

// the frames in the session's staging (all slots, packed) -> sizes_out [n_streams][n_rungs], sse_out [n_streams][n_rungs][3]: 28 bytes per
// (stream, rung) through probe_download
static int rd_probe_staged(pfv_enc_session *s, uint32_t *sizes_out, uint64_t *sse_out)
{
    pfv_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->n_streams * (size_t)s->n_rungs;
    const size_t sse_bytes = n * 3 * sizeof(uint64_t), size_bytes = n * sizeof(uint32_t);
    if (!s->rd_out) HIP_TRY(ctx, hipMalloc((void **)&s->rd_out, sse_bytes + size_bytes));
    int rc = rd_probe_launch(s, s->st_frames, (uint32_t *)((uint8_t *)s->rd_out + sse_bytes), s->rd_out, nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return probe_download(ctx, s->rd_out, n, sse_out, nullptr, sizes_out, nullptr);
}

extern "C" {

PFV_API int pfv_enc_probe_iframe_rd_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev)
{
    int rc = probe_dev_enter(s, frames_dev && sizes_dev && sse_dev, "pfv_enc_probe_iframe_rd_dev");
    return rc ? rc : rd_probe_launch(s, frames_dev, sizes_dev, sse_dev, stats_dev);
}
PFV_API int pfv_enc_probe_iframe_rd(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out)
{
    int rc = probe_host_enter(s, frames, sizes_out && sse_out, "pfv_enc_probe_iframe_rd");
    return rc ? rc : rd_probe_staged(s, sizes_out, sse_out);
}

}  // extern "C"
