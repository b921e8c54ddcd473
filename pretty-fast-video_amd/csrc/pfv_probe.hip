// pfv_probe.hip -- the i-frame size probe of an encoder session (pfv_enc_probe_iframe*): payload bytes of the window's frames as i-frames at every
// rung of the ladder, from one read of the frames.  Kernels: pfv_probe_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

// the kernels' accumulator: made and cleared by the first call, left clear by every k_probe_sizes
static int probe_acc(pfv_enc_session *s)
{
    pfv_ctx *ctx = s->ctx;
    if (s->probe_acc) return PFV_OK;
    if (ctx->capturing)
        return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_iframe_dev: the accumulator needs an allocation, which a graph recording cannot hold -- call once before pfv_graph_begin");
    const size_t bytes = (size_t)s->n_streams * (size_t)s->n_rungs * kProbeAcc * sizeof(uint32_t);
    HIP_TRY(ctx, hipMalloc((void **)&s->probe_acc, bytes));
    hipError_t e = hipMemsetAsync(s->probe_acc, 0, bytes, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(s->probe_acc);
        s->probe_acc = nullptr;
        return hip_fail(ctx, e, "pfv_enc_probe_iframe_dev");
    }
    return PFV_OK;
}

// slots [win_first, win_first + win_count): the same launches on shifted bases (see enc_launch); geometry and lane mapping are k_enc_iframe's
static int probe_launch(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev)
{
    pfv_ctx *ctx = s->ctx;
    int rc = probe_acc(s);
    if (rc) return rc;
    const size_t first = (size_t)s->win_first, R = (size_t)s->n_rungs;
    const size_t stride = s->in_stride ? s->in_stride : (size_t)s->geom.src_frame_bytes;
    const uint8_t *src = frames_dev + first * stride;
    const FrameGeom g = enc_win_geom(s, s->win_count, src);
    uint32_t *acc = s->probe_acc + first * R * kProbeAcc;
    if (use_small_grid(s->lane_mapping, g)) {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe<true, 16>), dim3(half_strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, src, (const QTab *)s->qtab_dev, s->n_rungs, acc);
        else hipLaunchKernelGGL((k_probe_iframe<false, 16>), dim3(half_strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, src, (const QTab *)s->qtab_dev, s->n_rungs, acc);
    } else {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe<true, 8>), dim3(strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, src, (const QTab *)s->qtab_dev, s->n_rungs, acc);
        else hipLaunchKernelGGL((k_probe_iframe<false, 8>), dim3(strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, src, (const QTab *)s->qtab_dev, s->n_rungs, acc);
    }
    hipLaunchKernelGGL(k_probe_sizes, dim3((unsigned)((size_t)s->win_count * R)), dim3(64), 0, ctx->stream, acc, sizes_dev + first * R,
                       stats_dev ? stats_dev + first * R * kProbeStats : (uint32_t *)nullptr);
    return launch_check(ctx, "k_probe_iframe / k_probe_sizes");
}

extern "C" {

PFV_API int pfv_enc_probe_iframe_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames_dev || !sizes_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_probe_iframe_dev: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return probe_launch(s, frames_dev, sizes_dev, stats_dev);
}

}  // extern "C"
// the frames in the session's staging (all slots, packed) -> sizes_out [n_streams][n_rungs]; synchronises
static int probe_staged(pfv_enc_session *s, uint32_t *sizes_out)
{
    pfv_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->n_streams * (size_t)s->n_rungs;
    if (!s->probe_sizes) HIP_TRY(ctx, hipMalloc((void **)&s->probe_sizes, n * sizeof(uint32_t)));
    int rc = probe_launch(s, s->st_frames, s->probe_sizes, nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIP_TRY(ctx, hipMemcpyAsync(sizes_out, s->probe_sizes, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}
extern "C" {

PFV_API int pfv_enc_probe_iframe(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames || !sizes_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_probe_iframe: null buffer");
    if (!enc_full_window(s)) return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_iframe: the host-buffer entry points work on all slots, packed (reset the window / frame stride)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_iframe: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = enc_staging(s);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s->st_frames, frames, (size_t)s->geom.src_frame_bytes * s->n_streams, hipMemcpyHostToDevice, ctx->stream));
    return probe_staged(s, sizes_out);
}

}  // extern "C"
