// pfv_quality.hip -- distortion measured where the frames lie: squared error per plane and per macroblock between two frames in device memory
// (pfv_frames_sse*), PSNR, and the sessions' own comparisons (the encoder's input against its closed-loop reconstruction, a decoder's
// framebuffer against reference frames).  Kernels: pfv_quality_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.
constexpr int kSseMapScratch = 6;   // pfv_ctx::scratch slot of the macroblock map when the caller passes none (no other entry point uses it)

// `g`: frame_geom(width, height, ...) as it comes -- src_frame_bytes / pad_frame_bytes are the layouts' own frame sizes
static SseOperand sse_operand(const FrameGeom &g, const uint8_t *base, int layout, size_t stride)
{
    SseOperand o;
    o.base = base;
    o.padded = layout == PFV_FRAME_PADDED ? 1 : 0;
    o.stride = stride ? (long)stride : (o.padded ? g.pad_frame_bytes : g.src_frame_bytes);
    o.vec = 0;
    if (((uintptr_t)base & 15) == 0 && o.stride % 16 == 0)
        for (int i = 0; i < 3; i++) {
            const PlaneGeom &p = g.p[i];
            if ((o.padded ? p.pw : p.w) % 16 == 0 && (o.padded ? p.pad_off : p.src_off) % 16 == 0) o.vec |= 1 << i;
        }
    return o;
}
// the two launches; sse [g.n_streams][3], mb [g.n_streams][g.mbs_per_frame]
static int sse_launch(pfv_ctx *ctx, const FrameGeom &g, const SseOperand &a, const SseOperand &b, uint64_t *sse, uint32_t *mb)
{
    hipLaunchKernelGGL(k_sse_mb, dim3(strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, a, b, mb);
    hipLaunchKernelGGL(k_sse_sum, dim3(3u * (unsigned)g.n_streams), dim3(kThreads), 0, ctx->stream, g, (const uint32_t *)mb, sse);
    return launch_check(ctx, "k_sse_mb / k_sse_sum");
}
static const char *const kSseNoAlloc = ": the macroblock map needs an allocation, which a graph recording cannot hold -- pass a map buffer, or call once before pfv_graph_begin";
// a session's own map, [n_streams][mbs_per_frame], made by the first call that passes none
static int session_map(pfv_ctx *ctx, uint32_t **map, size_t entries, const char *who)
{
    if (*map) return PFV_OK;
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, std::string(who) + kSseNoAlloc);
    HIP_TRY(ctx, hipMalloc((void **)map, entries * sizeof(uint32_t)));
    return PFV_OK;
}

// slots [win_first, win_first + win_count): the same launches on shifted bases (see enc_launch)
static int enc_distortion(pfv_enc_session *s, const uint8_t *frames_dev, uint64_t *sse_dev, uint32_t *mb_sse_dev)
{
    pfv_ctx *ctx = s->ctx;
    const size_t first = (size_t)s->win_first, mbs = (size_t)s->geom.mbs_per_frame;
    if (!mb_sse_dev) {
        int rc = session_map(ctx, &s->q_map, mbs * (size_t)s->n_streams, "pfv_enc_distortion_dev");
        if (rc) return rc;
        mb_sse_dev = s->q_map;
    }
    FrameGeom g = s->geom;
    g.n_streams = s->win_count;
    const size_t stride = s->in_stride ? s->in_stride : (size_t)g.src_frame_bytes;
    const SseOperand a = sse_operand(g, frames_dev + first * stride, PFV_FRAME_PACKED, stride);
    const SseOperand b = sse_operand(g, s->prev[s->cur] + first * (size_t)g.pad_frame_bytes, PFV_FRAME_PADDED, 0);
    return sse_launch(ctx, g, a, b, sse_dev + first * 3, mb_sse_dev + first * mbs);
}
// pfv_encoder's frame reports: the frame in the session's staging against the reconstruction the encode kernel has just written,
// and the sums on their way to the host behind it (the caller's next synchronisation of the context's stream delivers them)
static int enc_report_enqueue(pfv_enc_session *s)
{
    pfv_ctx *ctx = s->ctx;
    int rc = enc_distortion(s, s->st_frames, s->q_sse, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s->report_host, s->q_sse, (size_t)s->n_streams * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    return PFV_OK;
}
// switch the reports of a session on (host_sums: [n_streams][3], page-locked, owned by the caller) or off (nullptr)
static int enc_report_enable(pfv_enc_session *s, uint64_t *host_sums)
{
    pfv_ctx *ctx = s->ctx;
    if (host_sums) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "frame reports cannot be switched on while the context records a graph");
        int rc = enc_staging(s);
        if (!rc) rc = session_map(ctx, &s->q_map, (size_t)s->geom.mbs_per_frame * (size_t)s->n_streams, "frame reports");
        if (rc) return rc;
        if (!s->q_sse) HIP_TRY(ctx, hipMalloc((void **)&s->q_sse, (size_t)s->n_streams * 3 * sizeof(uint64_t)));
    }
    s->report_host = host_sums;
    return PFV_OK;
}

extern "C" {

PFV_API double pfv_psnr(uint64_t sse, uint64_t n_samples)
{
    if (n_samples == 0) return (double)NAN;
    if (sse == 0) return (double)INFINITY;
    return 10.0 * log10(255.0 * 255.0 * (double)n_samples / (double)sse);
}

PFV_API int pfv_frames_sse_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a_dev, int a_layout, size_t a_stride,
                               const uint8_t *b_dev, int b_layout, size_t b_stride, uint64_t *sse_dev, uint32_t *mb_sse_dev)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_sse_dev: width/height must be positive, even and fit u16");
    if (n_streams <= 0) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_sse_dev: n_streams must be positive");
    if (!a_dev || !b_dev || !sse_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_sse_dev: null buffer");
    if ((a_layout != PFV_FRAME_PACKED && a_layout != PFV_FRAME_PADDED) || (b_layout != PFV_FRAME_PACKED && b_layout != PFV_FRAME_PADDED))
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_sse_dev: layout must be PFV_FRAME_PACKED or PFV_FRAME_PADDED");
    const FrameGeom g = frame_geom(width, height, n_streams);
    if ((a_stride && a_stride < (size_t)(a_layout == PFV_FRAME_PADDED ? g.pad_frame_bytes : g.src_frame_bytes)) ||
        (b_stride && b_stride < (size_t)(b_layout == PFV_FRAME_PADDED ? g.pad_frame_bytes : g.src_frame_bytes)))
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_sse_dev: stride below the layout's frame size");
    if ((long)g.strips_per_frame * n_streams > 0x7fffffffL || (long)g.mbs_per_frame * n_streams > 0x7fffffffL)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_sse_dev: too many macroblocks for one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!mb_sse_dev) {
        const size_t bytes = (size_t)g.mbs_per_frame * (size_t)n_streams * sizeof(uint32_t);
        if (ctx->capturing && ctx->scratch_cap[kSseMapScratch] < bytes) return fail(ctx, PFV_ERR_STATE, std::string("pfv_frames_sse_dev") + kSseNoAlloc);
        void *map = nullptr;
        int rc = ensure_scratch(ctx, kSseMapScratch, bytes, &map);
        if (rc) return rc;
        mb_sse_dev = (uint32_t *)map;
    }
    return sse_launch(ctx, g, sse_operand(g, a_dev, a_layout, a_stride), sse_operand(g, b_dev, b_layout, b_stride), sse_dev, mb_sse_dev);
}

PFV_API int pfv_frames_sse(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a, const uint8_t *b, uint64_t *sse_out,
                           uint32_t *mb_sse_out)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535 || n_streams <= 0 || !a || !b || !sse_out)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_sse: bad argument (width/height positive and even, n_streams positive, no null buffer)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_sse: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t frames = pfv_frame_bytes(width, height) * (size_t)n_streams;
    const size_t n_map = (size_t)pfv_total_blocks(width, height) * (size_t)n_streams, sums = ((size_t)n_streams * 3 * sizeof(uint64_t) + 255) & ~(size_t)255;
    void *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = ensure_scratch(ctx, 0, frames, &d_a))) return rc;
    if (a != b && (rc = ensure_scratch(ctx, 2, frames, &d_b))) return rc;
    if ((rc = ensure_scratch(ctx, kSseMapScratch, sums + n_map * sizeof(uint32_t), &d_out))) return rc;   // the sums, then the map
    uint64_t *d_sse = (uint64_t *)d_out;
    uint32_t *d_map = (uint32_t *)((uint8_t *)d_out + sums);
    HIP_TRY(ctx, hipMemcpyAsync(d_a, a, frames, hipMemcpyHostToDevice, ctx->stream));
    if (a != b) HIP_TRY(ctx, hipMemcpyAsync(d_b, b, frames, hipMemcpyHostToDevice, ctx->stream));
    else d_b = d_a;
    if ((rc = pfv_frames_sse_dev(ctx, width, height, n_streams, (const uint8_t *)d_a, PFV_FRAME_PACKED, 0, (const uint8_t *)d_b, PFV_FRAME_PACKED, 0, d_sse, d_map))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(sse_out, d_sse, (size_t)n_streams * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (mb_sse_out) HIP_TRY(ctx, hipMemcpyAsync(mb_sse_out, d_map, n_map * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

PFV_API int pfv_enc_distortion_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint64_t *sse_dev, uint32_t *mb_sse_dev)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames_dev || !sse_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_distortion_dev: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return enc_distortion(s, frames_dev, sse_dev, mb_sse_dev);
}

PFV_API int pfv_dec_distortion_dev(pfv_dec_session *s, const uint8_t *frames_dev, uint64_t *sse_dev, uint32_t *mb_sse_dev)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames_dev || !sse_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_distortion_dev: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t first = (size_t)s->win_first, mbs = (size_t)s->geom.mbs_per_frame;
    if (!mb_sse_dev) {
        int rc = session_map(ctx, &s->q_map, mbs * (size_t)s->n_streams, "pfv_dec_distortion_dev");
        if (rc) return rc;
        mb_sse_dev = s->q_map;
    }
    FrameGeom g = s->geom;
    g.n_streams = s->win_count;
    const size_t stride = s->out_stride ? s->out_stride : (size_t)g.src_frame_bytes;
    const SseOperand a = sse_operand(g, frames_dev + first * stride, PFV_FRAME_PACKED, stride);
    const SseOperand b = sse_operand(g, s->fb[s->cur] + first * (size_t)g.pad_frame_bytes, PFV_FRAME_PADDED, 0);
    return sse_launch(ctx, g, a, b, sse_dev + first * 3, mb_sse_dev + first * mbs);
}

}  // extern "C"
