// pfv_ingest.hip -- planar frames from RGB / RGBA / BGRA pictures: pictures in device or host memory (pfv_frames_from_rgb*) and the pictures of
// an encoder session's window into a packed frame buffer the session owns (pfv_enc_ingest_rgb_dev).  pfv_encoder's switch
// (pfv_encoder_set_input_rgb) is in pfv_stream_objects.hip and launches through ingest_launch.  Kernel: pfv_ingest_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

static bool chroma_mode_ok(int chroma) { return chroma == PFV_CHROMA_POINT || chroma == PFV_CHROMA_BOX; }

template <int FMT>
static void ingest_launch_fmt(pfv_ctx *ctx, int chroma, dim3 grid, int w, int h, const IngestSrc &s, uint8_t *dst, long dst_stride, int groups_x, unsigned n_columns, int wide)
{
    if (chroma == PFV_CHROMA_BOX) hipLaunchKernelGGL((k_ingest_rgb<FMT, kChromaBox>), grid, dim3(kThreads), 0, ctx->stream, w, h, s, dst, dst_stride, groups_x, n_columns, wide);
    else hipLaunchKernelGGL((k_ingest_rgb<FMT, kChromaPoint>), grid, dim3(kThreads), 0, ctx->stream, w, h, s, dst, dst_stride, groups_x, n_columns, wide);
}

// one launch; format and chroma are valid, pitch, stride and dst_stride final.
// The wide path needs every 8- / 16-byte load and every 8- / 4-byte store of a lane to be aligned: a width that is a multiple of 8 (luma rows
// are then 8-byte aligned inside a frame, chroma rows and the U and V planes 4-byte aligned); source base, pitch and stride to 8 bytes (RGB8) or
// 16 (the 4-byte formats); destination base and stride to 8 bytes.
static int ingest_launch(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src, int format, size_t pitch, size_t stride, uint8_t *dst,
                         size_t dst_stride, int chroma)
{
    if (n_streams > 65535) return fail(ctx, PFV_ERR_BAD_ARG, "k_ingest_rgb: too many streams for one launch");
    const size_t sa = format == PFV_PIX_RGB8 ? 8 : 16;
    const bool wide = width % 8 == 0 && (uintptr_t)src % sa == 0 && pitch % sa == 0 && stride % sa == 0 && (uintptr_t)dst % 8 == 0 && dst_stride % 8 == 0;
    const int groups_x = (width + 7) / 8;
    const unsigned n_columns = (unsigned)groups_x * (unsigned)((height / 2 + kIngestPairs - 1) / kIngestPairs);   // columns of kIngestPairs groups
    const dim3 grid((n_columns + kThreads - 1) / kThreads, (unsigned)n_streams);
    const IngestSrc s{src, (long)pitch, (long)stride};
    if (format == PFV_PIX_RGB8) ingest_launch_fmt<kPixRgb8>(ctx, chroma, grid, width, height, s, dst, (long)dst_stride, groups_x, n_columns, wide ? 1 : 0);
    else if (format == PFV_PIX_RGBA8) ingest_launch_fmt<kPixRgba8>(ctx, chroma, grid, width, height, s, dst, (long)dst_stride, groups_x, n_columns, wide ? 1 : 0);
    else ingest_launch_fmt<kPixBgra8>(ctx, chroma, grid, width, height, s, dst, (long)dst_stride, groups_x, n_columns, wide ? 1 : 0);
    return launch_check(ctx, "k_ingest_rgb");
}

extern "C" {

PFV_API int pfv_frames_from_rgb_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src_dev, int format, size_t src_pitch, size_t src_stride,
                                    uint8_t *dst_dev, size_t dst_stride, int chroma)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_from_rgb_dev: width/height must be positive, even and fit u16");
    if (n_streams <= 0) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_from_rgb_dev: n_streams must be positive");
    if (!src_dev || !dst_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_from_rgb_dev: null buffer");
    if (!chroma_mode_ok(chroma)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_from_rgb_dev: chroma must be PFV_CHROMA_POINT or PFV_CHROMA_BOX");
    int rc = present_layout(ctx, "pfv_frames_from_rgb_dev", width, height, format, &src_pitch, &src_stride);
    if (rc) return rc;
    const size_t fb = pfv_frame_bytes(width, height);
    if (dst_stride && dst_stride < fb) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_from_rgb_dev: destination stride below pfv_frame_bytes");
    if (!dst_stride) dst_stride = fb;
    // first picture .. end of the last row of the last one, and first frame .. end of the last one
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + (size_t)(n_streams - 1) * src_stride + (size_t)(height - 1) * src_pitch + pfv_rgb_row_bytes(width, format);
    const uintptr_t d0 = (uintptr_t)dst_dev, d1 = d0 + (size_t)(n_streams - 1) * dst_stride + fb;
    if (s0 < d1 && d0 < s1) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_from_rgb_dev: source and destination overlap");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ingest_launch(ctx, width, height, n_streams, src_dev, format, src_pitch, src_stride, dst_dev, dst_stride, chroma);
}

PFV_API int pfv_frames_from_rgb(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src, uint8_t *dst, int format, int chroma)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535 || n_streams <= 0 || !src || !dst || !pix_format_ok(format) ||
        !chroma_mode_ok(chroma))
        return fail(ctx, PFV_ERR_BAD_ARG,
                    "pfv_frames_from_rgb: bad argument (width/height positive and even, n_streams positive, no null buffer, a PFV_PIX_* format, a PFV_CHROMA_* mode)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_from_rgb: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t frames = pfv_frame_bytes(width, height) * (size_t)n_streams, pics = pfv_rgb_row_bytes(width, format) * (size_t)height * (size_t)n_streams;
    void *d_src = nullptr, *d_dst = nullptr;
    int rc;
    if ((rc = ensure_scratch(ctx, 2, pics, &d_src))) return rc;
    if ((rc = ensure_scratch(ctx, 0, frames, &d_dst))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_src, src, pics, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pfv_frames_from_rgb_dev(ctx, width, height, n_streams, (const uint8_t *)d_src, format, 0, 0, (uint8_t *)d_dst, 0, chroma))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_dst, frames, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

PFV_API int pfv_enc_ingest_rgb_dev(pfv_enc_session *s, const uint8_t *pictures_dev, int format, size_t pitch, size_t stride, int chroma,
                                   const uint8_t **frames_dev_out)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!pictures_dev || !frames_dev_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_ingest_rgb_dev: null buffer");
    if (!chroma_mode_ok(chroma)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_ingest_rgb_dev: chroma must be PFV_CHROMA_POINT or PFV_CHROMA_BOX");
    int rc = present_layout(ctx, "pfv_enc_ingest_rgb_dev", s->width, s->height, format, &pitch, &stride);
    if (rc) return rc;
    if (s->in_stride) return fail(ctx, PFV_ERR_STATE, "pfv_enc_ingest_rgb_dev: the session's frame buffer is packed (reset pfv_enc_session_set_frame_stride; GOP-batched pictures use the picture stride)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t fb = (size_t)s->geom.src_frame_bytes;
    if (!s->ingest_frames) {
        if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_enc_ingest_rgb_dev: the first call allocates the session's frame buffer, which a graph recording cannot -- call once before pfv_graph_begin");
        HIP_TRY(ctx, hipMalloc((void **)&s->ingest_frames, fb * (size_t)s->n_streams));
    }
    *frames_dev_out = s->ingest_frames;
    return ingest_launch(ctx, s->width, s->height, s->win_count, pictures_dev + (size_t)s->win_first * stride, format, pitch, stride,
                         s->ingest_frames + (size_t)s->win_first * fb, fb, chroma);
}

}  // extern "C"
