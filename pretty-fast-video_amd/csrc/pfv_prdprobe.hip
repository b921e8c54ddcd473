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

// slots [win_first, win_first + win_count), as pprobe_launch
static int prd_probe_launch(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev)
{
    pfv_ctx *ctx = s->ctx;
    int rc = prd_probe_acc(s);
    if (rc) return rc;
    const size_t first = (size_t)s->win_first, R = (size_t)s->n_rungs;
    const size_t stride = s->in_stride ? s->in_stride : (size_t)s->geom.src_frame_bytes;
    const uint8_t *src = frames_dev + first * stride;
    const FrameGeom g = enc_win_geom(s, s->win_count, src);
    const uint8_t *ref = s->prev[s->cur] + first * (size_t)s->geom.pad_frame_bytes;
    uint32_t *acc = s->pprobe_acc + first * R * kPProbeAcc;
    const float *min_err = reinterpret_cast<const float *>(s->pprobe_acc + (size_t)s->n_streams * R * kPProbeAcc);
    unsigned long long *sse_acc = (unsigned long long *)s->rd_acc + first * R * 3;
    const QTab *qt = (const QTab *)s->qtab_dev;
    if (s->flt) hipLaunchKernelGGL(k_probe_pframe_rd<true>, dim3(penc_blocks(ctx, g)), dim3(kThreads), 0, ctx->stream, g, src, ref, qt, s->n_rungs, min_err, -2, acc, sse_acc);
    else hipLaunchKernelGGL(k_probe_pframe_rd<false>, dim3(penc_blocks(ctx, g)), dim3(kThreads), 0, ctx->stream, g, src, ref, qt, s->n_rungs, min_err, -2, acc, sse_acc);
    hipLaunchKernelGGL(k_pprobe_rd_sizes, dim3((unsigned)((size_t)s->win_count * R)), dim3(64), 0, ctx->stream, acc, sizes_dev + first * R,
                       stats_dev ? stats_dev + first * R * kPProbeStats : (uint32_t *)nullptr, sse_acc, (unsigned long long *)sse_dev + first * R * 3);
    return launch_check(ctx, "k_probe_pframe_rd / k_pprobe_rd_sizes");
}

extern "C" {

PFV_API int pfv_enc_probe_pframe_rd_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames_dev || !sizes_dev || !sse_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_probe_pframe_rd_dev: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return prd_probe_launch(s, frames_dev, sizes_dev, sse_dev, stats_dev);
}

}  // extern "C"
// the frames in the session's staging (all slots, packed) -> sizes_out [n_streams][n_rungs], sse_out [n_streams][n_rungs][3] and, where asked
// for, stats_out [n_streams][n_rungs][kPProbeStats]; one download of 28 bytes per (stream, rung) -- the sums first, so that both parts stay
// aligned --, the counts behind them where asked for, and one synchronisation
static int prd_probe_staged(pfv_enc_session *s, uint32_t *sizes_out, uint64_t *sse_out, uint32_t *stats_out = nullptr)
{
    pfv_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->n_streams * (size_t)s->n_rungs;
    const size_t sse_bytes = n * 3 * sizeof(uint64_t), size_bytes = n * sizeof(uint32_t), stat_bytes = n * kPProbeStats * sizeof(uint32_t);
    if (!s->prd_out) HIP_TRY(ctx, hipMalloc((void **)&s->prd_out, sse_bytes + size_bytes + stat_bytes));
    const size_t bytes = sse_bytes + size_bytes + (stats_out ? stat_bytes : 0);
    std::vector<uint8_t> host(bytes);
    uint32_t *sizes_dev = (uint32_t *)((uint8_t *)s->prd_out + sse_bytes);
    int rc = prd_probe_launch(s, s->st_frames, sizes_dev, s->prd_out, stats_out ? sizes_dev + n : nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), s->prd_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(sse_out, host.data(), sse_bytes);
    memcpy(sizes_out, host.data() + sse_bytes, size_bytes);
    if (stats_out) memcpy(stats_out, host.data() + sse_bytes + size_bytes, stat_bytes);
    return PFV_OK;
}
extern "C" {

PFV_API int pfv_enc_probe_pframe_rd(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames || !sizes_out || !sse_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_probe_pframe_rd: null buffer");
    if (!enc_full_window(s)) return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_pframe_rd: the host-buffer entry points work on all slots, packed (reset the window / frame stride)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_pframe_rd: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = enc_staging(s);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s->st_frames, frames, (size_t)s->geom.src_frame_bytes * s->n_streams, hipMemcpyHostToDevice, ctx->stream));
    return prd_probe_staged(s, sizes_out, sse_out);
}

}  // extern "C"
