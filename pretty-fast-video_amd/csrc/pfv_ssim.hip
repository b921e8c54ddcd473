// pfv_ssim.hip -- structural similarity measured where the frames lie: the SSIM sums per plane and per macroblock between two frames in device
// memory (pfv_frames_ssim*), the mean from them (pfv_ssim), and the sessions' own comparisons, with the operands, window and strides of the
// distortion entry points (pfv_quality.hip).  Kernels: pfv_ssim_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.
constexpr int kSsimMapScratch = 8;   // pfv_ctx::scratch slot of the macroblock map when the caller passes none (no other entry point uses it)

// the two launches; ssim [g.n_streams][3], mb [g.n_streams][g.mbs_per_frame]
static int ssim_launch(pfv_ctx *ctx, const FrameGeom &g, const SseOperand &a, const SseOperand &b, int64_t *ssim, int32_t *mb)
{
    hipLaunchKernelGGL(k_ssim_mb, dim3(strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, a, b, mb);
    hipLaunchKernelGGL(k_ssim_sum, dim3(3u * (unsigned)g.n_streams), dim3(kThreads), 0, ctx->stream, g, (const int32_t *)mb, ssim);
    return launch_check(ctx, "k_ssim_mb / k_ssim_sum");
}

// slots [win_first, win_first + win_count): the same launches on shifted bases (see enc_distortion)
static int enc_ssim(pfv_enc_session *s, const uint8_t *frames_dev, int64_t *ssim_dev, int32_t *mb_dev, const char *who)
{
    pfv_ctx *ctx = s->ctx;
    const size_t first = (size_t)s->win_first, mbs = (size_t)s->geom.mbs_per_frame;
    if (!mb_dev) {
        int rc = session_map(ctx, (uint32_t **)&s->ssim_map, mbs * (size_t)s->n_streams, who);
        if (rc) return rc;
        mb_dev = s->ssim_map;
    }
    FrameGeom g = s->geom;
    g.n_streams = s->win_count;
    const size_t stride = s->in_stride ? s->in_stride : (size_t)g.src_frame_bytes;
    const SseOperand a = sse_operand(g, frames_dev + first * stride, PFV_FRAME_PACKED, stride);
    const SseOperand b = sse_operand(g, s->prev[s->cur] + first * (size_t)g.pad_frame_bytes, PFV_FRAME_PADDED, 0);
    return ssim_launch(ctx, g, a, b, ssim_dev + first * 3, mb_dev + first * mbs);
}
// pfv_encoder's frame SSIM: the frame in the session's staging against the reconstruction the encode kernel has just written, and the sums
// on their way to the host behind it (the caller's next synchronisation of the context's stream delivers them)
static int enc_ssim_enqueue(pfv_enc_session *s)
{
    pfv_ctx *ctx = s->ctx;
    int rc = enc_ssim(s, s->st_frames, s->ssim_sums, nullptr, "frame SSIM");
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s->ssim_host, s->ssim_sums, (size_t)s->n_streams * 3 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    return PFV_OK;
}
// switch the frame SSIM of a session on (host_sums: [n_streams][3], page-locked, owned by the caller) or off (nullptr)
static int enc_ssim_enable(pfv_enc_session *s, int64_t *host_sums)
{
    pfv_ctx *ctx = s->ctx;
    if (host_sums) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "frame SSIM cannot be switched on while the context records a graph");
        int rc = enc_staging(s);
        if (!rc) rc = session_map(ctx, (uint32_t **)&s->ssim_map, (size_t)s->geom.mbs_per_frame * (size_t)s->n_streams, "frame SSIM");
        if (rc) return rc;
        if (!s->ssim_sums) HIP_TRY(ctx, hipMalloc((void **)&s->ssim_sums, (size_t)s->n_streams * 3 * sizeof(int64_t)));
    }
    s->ssim_host = host_sums;
    return PFV_OK;
}

extern "C" {

PFV_API double pfv_ssim(int64_t q24_sum, uint64_t windows)
{
    if (windows == 0) return (double)NAN;
    return (double)q24_sum / (16777216.0 * (double)windows);
}

PFV_API int pfv_ssim_windows(int width, int height, uint32_t out[3])
{
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535 || !out) return PFV_ERR_BAD_ARG;
    for (int i = 0; i < 3; i++) {
        const int bw = (i ? width / 2 : width) >> 2, bh = (i ? height / 2 : height) >> 2;
        out[i] = (uint32_t)std::max(0, bw - 1) * (uint32_t)std::max(0, bh - 1);
    }
    return PFV_OK;
}

PFV_API int pfv_frames_ssim_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a_dev, int a_layout, size_t a_stride,
                                const uint8_t *b_dev, int b_layout, size_t b_stride, int64_t *ssim_q24_dev, int32_t *mb_ssim_q24_dev)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_ssim_dev: width/height must be positive, even and fit u16");
    if (n_streams <= 0) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_ssim_dev: n_streams must be positive");
    if (!a_dev || !b_dev || !ssim_q24_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_ssim_dev: null buffer");
    if ((a_layout != PFV_FRAME_PACKED && a_layout != PFV_FRAME_PADDED) || (b_layout != PFV_FRAME_PACKED && b_layout != PFV_FRAME_PADDED))
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_ssim_dev: layout must be PFV_FRAME_PACKED or PFV_FRAME_PADDED");
    const FrameGeom g = frame_geom(width, height, n_streams);
    if ((a_stride && a_stride < (size_t)(a_layout == PFV_FRAME_PADDED ? g.pad_frame_bytes : g.src_frame_bytes)) ||
        (b_stride && b_stride < (size_t)(b_layout == PFV_FRAME_PADDED ? g.pad_frame_bytes : g.src_frame_bytes)))
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_ssim_dev: stride below the layout's frame size");
    if ((long)g.strips_per_frame * n_streams > 0x7fffffffL || (long)g.mbs_per_frame * n_streams > 0x7fffffffL)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_ssim_dev: too many macroblocks for one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!mb_ssim_q24_dev) {
        const size_t bytes = (size_t)g.mbs_per_frame * (size_t)n_streams * sizeof(int32_t);
        if (ctx->capturing && ctx->scratch_cap[kSsimMapScratch] < bytes) return fail(ctx, PFV_ERR_STATE, std::string("pfv_frames_ssim_dev") + kSseNoAlloc);
        void *map = nullptr;
        int rc = ensure_scratch(ctx, kSsimMapScratch, bytes, &map);
        if (rc) return rc;
        mb_ssim_q24_dev = (int32_t *)map;
    }
    return ssim_launch(ctx, g, sse_operand(g, a_dev, a_layout, a_stride), sse_operand(g, b_dev, b_layout, b_stride), ssim_q24_dev, mb_ssim_q24_dev);
}

PFV_API int pfv_frames_ssim(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a, const uint8_t *b, int64_t *ssim_q24_out,
                            int32_t *mb_out)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535 || n_streams <= 0 || !a || !b || !ssim_q24_out)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_ssim: bad argument (width/height positive and even, n_streams positive, no null buffer)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_ssim: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t frames = pfv_frame_bytes(width, height) * (size_t)n_streams;
    const size_t n_map = (size_t)pfv_total_blocks(width, height) * (size_t)n_streams, sums = ((size_t)n_streams * 3 * sizeof(int64_t) + 255) & ~(size_t)255;
    void *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = ensure_scratch(ctx, 0, frames, &d_a))) return rc;
    if (a != b && (rc = ensure_scratch(ctx, 2, frames, &d_b))) return rc;
    if ((rc = ensure_scratch(ctx, kSsimMapScratch, sums + n_map * sizeof(int32_t), &d_out))) return rc;   // the sums, then the map
    int64_t *d_sums = (int64_t *)d_out;
    int32_t *d_map = (int32_t *)((uint8_t *)d_out + sums);
    HIP_TRY(ctx, hipMemcpyAsync(d_a, a, frames, hipMemcpyHostToDevice, ctx->stream));
    if (a != b) HIP_TRY(ctx, hipMemcpyAsync(d_b, b, frames, hipMemcpyHostToDevice, ctx->stream));
    else d_b = d_a;
    if ((rc = pfv_frames_ssim_dev(ctx, width, height, n_streams, (const uint8_t *)d_a, PFV_FRAME_PACKED, 0, (const uint8_t *)d_b, PFV_FRAME_PACKED, 0, d_sums, d_map))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ssim_q24_out, d_sums, (size_t)n_streams * 3 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (mb_out) HIP_TRY(ctx, hipMemcpyAsync(mb_out, d_map, n_map * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

PFV_API int pfv_enc_ssim_dev(pfv_enc_session *s, const uint8_t *frames_dev, int64_t *ssim_q24_dev, int32_t *mb_dev)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames_dev || !ssim_q24_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_ssim_dev: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return enc_ssim(s, frames_dev, ssim_q24_dev, mb_dev, "pfv_enc_ssim_dev");
}

PFV_API int pfv_dec_ssim_dev(pfv_dec_session *s, const uint8_t *frames_dev, int64_t *ssim_q24_dev, int32_t *mb_dev)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames_dev || !ssim_q24_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_ssim_dev: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t first = (size_t)s->win_first, mbs = (size_t)s->geom.mbs_per_frame;
    if (!mb_dev) {
        int rc = session_map(ctx, (uint32_t **)&s->ssim_map, mbs * (size_t)s->n_streams, "pfv_dec_ssim_dev");
        if (rc) return rc;
        mb_dev = s->ssim_map;
    }
    FrameGeom g = s->geom;
    g.n_streams = s->win_count;
    const size_t stride = s->out_stride ? s->out_stride : (size_t)g.src_frame_bytes;
    const SseOperand a = sse_operand(g, frames_dev + first * stride, PFV_FRAME_PACKED, stride);
    const SseOperand b = sse_operand(g, s->fb[s->cur] + first * (size_t)g.pad_frame_bytes, PFV_FRAME_PADDED, 0);
    return ssim_launch(ctx, g, a, b, ssim_q24_dev + first * 3, mb_dev + first * mbs);
}

}  // extern "C"
