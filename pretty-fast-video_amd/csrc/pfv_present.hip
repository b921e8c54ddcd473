// pfv_present.hip -- RGB / RGBA / BGRA pictures from planar frames: frames in device or host memory (pfv_frames_to_rgb*), a decoder session's
// pictures on request (pfv_dec_get_frame_rgb*) and with every decode call (pfv_dec_set_output_rgb_dev), and pfv_decoder's switch
// (pfv_decoder_set_output_rgb).  Kernel: pfv_present_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

static bool pix_format_ok(int format) { return format == PFV_PIX_RGB8 || format == PFV_PIX_RGBA8 || format == PFV_PIX_BGRA8; }

// pitch / stride with their defaults, or PFV_ERR_BAD_ARG; `what` names the entry point
static int present_layout(pfv_ctx *ctx, const char *what, int width, int height, int format, size_t *pitch, size_t *stride)
{
    const size_t row = pfv_rgb_row_bytes(width, format);
    if (!row) return fail(ctx, PFV_ERR_BAD_ARG, std::string(what) + ": format must be PFV_PIX_RGB8, _RGBA8 or _BGRA8");
    if (*pitch && *pitch < row) return fail(ctx, PFV_ERR_BAD_ARG, std::string(what) + ": pitch below pfv_rgb_row_bytes");
    if (!*pitch) *pitch = row;
    if (*stride && *stride < *pitch * (size_t)height) return fail(ctx, PFV_ERR_BAD_ARG, std::string(what) + ": stride below pitch x height");
    if (!*stride) *stride = *pitch * (size_t)height;
    return PFV_OK;
}

// one launch.  `g`: frame_geom(width, height, n_streams) as it comes; pitch and stride are final (present_layout).
// The wide path needs every dword a lane loads and every 12- / 16-byte span it stores to be aligned: luma and chroma plane bases and row
// strides and the stream stride to 4 bytes; destination base, pitch and stride to 4 bytes (RGB8) or 16 (the 4-byte formats).
static int present_launch(pfv_ctx *ctx, const FrameGeom &g, const SseOperand &src, uint8_t *dst, int format, size_t pitch, size_t stride)
{
    if (g.n_streams > 65535) return fail(ctx, PFV_ERR_BAD_ARG, "k_present_rgb: too many streams for one launch");
    bool wide = ((uintptr_t)src.base & 3) == 0 && src.stride % 4 == 0;
    for (int i = 0; i < 3; i++) {
        const PlaneGeom &p = g.p[i];
        wide = wide && (src.padded ? p.pw : p.w) % 4 == 0 && (src.padded ? p.pad_off : p.src_off) % 4 == 0;
    }
    const size_t da = format == PFV_PIX_RGB8 ? 4 : 16;
    wide = wide && (uintptr_t)dst % da == 0 && pitch % da == 0 && stride % da == 0;
    const int groups_x = (g.p[0].w + 3) / 4;
    const unsigned n_groups = (unsigned)groups_x * (unsigned)((g.p[0].h / 2 + kPresentPairs - 1) / kPresentPairs);   // columns of kPresentPairs groups
    const dim3 grid((n_groups + kThreads - 1) / kThreads, (unsigned)g.n_streams);
    const PresentDst d{dst, (long)pitch, (long)stride};
    if (format == PFV_PIX_RGB8) hipLaunchKernelGGL((k_present_rgb<kPixRgb8>), grid, dim3(kThreads), 0, ctx->stream, g, src, d, groups_x, n_groups, wide ? 1 : 0);
    else if (format == PFV_PIX_RGBA8) hipLaunchKernelGGL((k_present_rgb<kPixRgba8>), grid, dim3(kThreads), 0, ctx->stream, g, src, d, groups_x, n_groups, wide ? 1 : 0);
    else hipLaunchKernelGGL((k_present_rgb<kPixBgra8>), grid, dim3(kThreads), 0, ctx->stream, g, src, d, groups_x, n_groups, wide ? 1 : 0);
    return launch_check(ctx, "k_present_rgb");
}

// the packed scratch a deblocked picture passes through on its way to k_present_rgb; allocated outside decode calls only
static int dec_present_scratch(pfv_dec_session *s, const char *what)
{
    pfv_ctx *ctx = s->ctx;
    if (s->db_scratch) return PFV_OK;
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, std::string(what) + ": the deblocked picture needs scratch, which a graph recording cannot allocate -- call once before pfv_graph_begin");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc((void **)&s->db_scratch, (size_t)s->geom.src_frame_bytes * s->n_streams));
    return PFV_OK;
}

// Slots [first, first + count) of a decoder session as an operand (*g with n_streams = count), holding what pfv_dec_get_frame_dev would return
// now.  Deblocking off: the padded framebuffer, read where it lies.  On: the filtered packed frames -- `filtered` (frames `filtered_stride`
// apart, indexed by slot) when the caller has just produced them, else one k_deblock into the session's scratch first.
static int dec_shown_operand(pfv_dec_session *s, int first, int count, const uint8_t *filtered, size_t filtered_stride, FrameGeom *g, SseOperand *src)
{
    *g = s->geom;
    g->n_streams = count;
    const size_t fb = (size_t)g->src_frame_bytes;
    if (!s->db_mode) {
        *src = sse_operand(*g, s->fb[s->cur] + (size_t)first * (size_t)g->pad_frame_bytes, PFV_FRAME_PADDED, 0);
    } else if (filtered) {
        const size_t fs = filtered_stride ? filtered_stride : fb;
        *src = sse_operand(*g, filtered + (size_t)first * fs, PFV_FRAME_PACKED, fs);
    } else {
        if (!s->db_scratch) return fail(s->ctx, PFV_ERR_STATE, "RGB / resized output of a deblocked picture: the session's scratch is missing");
        const int rc = dec_deblock_win(s, first, count, s->db_scratch, 0);
        if (rc) return rc;
        *src = sse_operand(*g, s->db_scratch + (size_t)first * fb, PFV_FRAME_PACKED, 0);
    }
    return PFV_OK;
}
// ... as RGB pictures
static int dec_present_win(pfv_dec_session *s, int first, int count, const uint8_t *filtered, size_t filtered_stride, uint8_t *dst, int format, size_t pitch,
                           size_t stride)
{
    FrameGeom g;
    SseOperand src;
    const int rc = dec_shown_operand(s, first, count, filtered, filtered_stride, &g, &src);
    if (rc) return rc;
    return present_launch(s->ctx, g, src, dst + (size_t)first * stride, format, pitch, stride);
}
// ... as frames of a scaler's destination size (packed, `stride` apart, indexed by slot)
static int dec_scaled_win(pfv_dec_session *s, pfv_scaler *sc, int first, int count, const uint8_t *filtered, size_t filtered_stride, uint8_t *dst, size_t stride)
{
    FrameGeom g;
    SseOperand src;
    const int rc = dec_shown_operand(s, first, count, filtered, filtered_stride, &g, &src);
    if (rc) return rc;
    return scale_launch(sc, count, src.base, src.padded ? PFV_FRAME_PADDED : PFV_FRAME_PACKED, (size_t)src.stride, dst + (size_t)first * stride, stride);
}
// the decode calls' share (dec_step): the window's pictures into the output of pfv_dec_set_output_rgb_dev, its resized frames into the output of
// pfv_dec_set_output_scaled_dev -- from one operand: a deblocked picture that no planar output takes is filtered once for both
static int dec_present_step(pfv_dec_session *s)
{
    FrameGeom g;
    SseOperand src;
    int rc = dec_shown_operand(s, s->win_first, s->win_count, s->frames_out, s->out_stride, &g, &src);
    if (!rc && s->rgb_out) rc = present_launch(s->ctx, g, src, s->rgb_out + (size_t)s->win_first * s->rgb_stride, s->rgb_format, s->rgb_pitch, s->rgb_stride);
    if (!rc && s->scaled_out)
        rc = scale_launch(s->scaled_sc, s->win_count, src.base, src.padded ? PFV_FRAME_PADDED : PFV_FRAME_PACKED, (size_t)src.stride,
                          s->scaled_out + (size_t)s->win_first * s->scaled_stride, s->scaled_stride);
    return rc;
}

extern "C" {

PFV_API size_t pfv_rgb_row_bytes(int width, int format)
{
    if (width <= 0 || !pix_format_ok(format)) return 0;
    return (size_t)width * (format == PFV_PIX_RGB8 ? 3u : 4u);
}

PFV_API int pfv_frames_to_rgb_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src_dev, int src_layout, size_t src_stride,
                                  uint8_t *dst_dev, int format, size_t dst_pitch, size_t dst_stride)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_to_rgb_dev: width/height must be positive, even and fit u16");
    if (n_streams <= 0) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_to_rgb_dev: n_streams must be positive");
    if (!src_dev || !dst_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_to_rgb_dev: null buffer");
    if (src_layout != PFV_FRAME_PACKED && src_layout != PFV_FRAME_PADDED)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_to_rgb_dev: layout must be PFV_FRAME_PACKED or PFV_FRAME_PADDED");
    int rc = present_layout(ctx, "pfv_frames_to_rgb_dev", width, height, format, &dst_pitch, &dst_stride);
    if (rc) return rc;
    const FrameGeom g = frame_geom(width, height, n_streams);
    const size_t src_frame = (size_t)(src_layout == PFV_FRAME_PADDED ? g.pad_frame_bytes : g.src_frame_bytes);
    if (src_stride && src_stride < src_frame) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_to_rgb_dev: source stride below the layout's frame size");
    // first frame .. end of the last one, and first picture .. end of the last row of the last one
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + (size_t)(n_streams - 1) * (src_stride ? src_stride : src_frame) + src_frame;
    const uintptr_t d0 = (uintptr_t)dst_dev, d1 = d0 + (size_t)(n_streams - 1) * dst_stride + (size_t)(height - 1) * dst_pitch + pfv_rgb_row_bytes(width, format);
    if (s0 < d1 && d0 < s1) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_to_rgb_dev: source and destination overlap");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return present_launch(ctx, g, sse_operand(g, src_dev, src_layout, src_stride), dst_dev, format, dst_pitch, dst_stride);
}

PFV_API int pfv_frames_to_rgb(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src, uint8_t *dst, int format)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535 || n_streams <= 0 || !src || !dst || !pix_format_ok(format))
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_to_rgb: bad argument (width/height positive and even, n_streams positive, no null buffer, a PFV_PIX_* format)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_to_rgb: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t frames = pfv_frame_bytes(width, height) * (size_t)n_streams, pics = pfv_rgb_row_bytes(width, format) * (size_t)height * (size_t)n_streams;
    void *d_src = nullptr, *d_dst = nullptr;
    int rc;
    if ((rc = ensure_scratch(ctx, 0, frames, &d_src))) return rc;
    if ((rc = ensure_scratch(ctx, 2, pics, &d_dst))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_src, src, frames, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pfv_frames_to_rgb_dev(ctx, width, height, n_streams, (const uint8_t *)d_src, PFV_FRAME_PACKED, 0, (uint8_t *)d_dst, format, 0, 0))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_dst, pics, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

PFV_API int pfv_dec_get_frame_rgb_dev(pfv_dec_session *s, uint8_t *dst_dev, int format, size_t pitch, size_t stride)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!dst_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_get_frame_rgb_dev: null buffer");
    int rc = present_layout(ctx, "pfv_dec_get_frame_rgb_dev", s->width, s->height, format, &pitch, &stride);
    if (rc) return rc;
    if (s->db_mode && (rc = dec_present_scratch(s, "pfv_dec_get_frame_rgb_dev"))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dec_present_win(s, 0, s->n_streams, nullptr, 0, dst_dev, format, pitch, stride);
}

PFV_API int pfv_dec_get_frame_rgb(pfv_dec_session *s, uint8_t *dst_host, int format)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!dst_host) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_get_frame_rgb: null buffer");
    if (!pix_format_ok(format)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_get_frame_rgb: format must be PFV_PIX_RGB8, _RGBA8 or _BGRA8");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_dec_get_frame_rgb: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!s->st_rgb) HIP_TRY(ctx, hipMalloc((void **)&s->st_rgb, (size_t)s->width * s->height * 4 * s->n_streams));   // holds any format
    int rc = pfv_dec_get_frame_rgb_dev(s, s->st_rgb, format, 0, 0);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dst_host, s->st_rgb, pfv_rgb_row_bytes(s->width, format) * (size_t)s->height * s->n_streams, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

PFV_API int pfv_dec_set_output_rgb_dev(pfv_dec_session *s, uint8_t *dst_dev, int format, size_t pitch, size_t stride)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    if (!dst_dev) {
        s->rgb_out = nullptr;
        return PFV_OK;
    }
    int rc = present_layout(s->ctx, "pfv_dec_set_output_rgb_dev", s->width, s->height, format, &pitch, &stride);
    if (rc) return rc;
    if (s->db_mode && (rc = dec_present_scratch(s, "pfv_dec_set_output_rgb_dev"))) return rc;
    s->rgb_out = dst_dev; s->rgb_format = format; s->rgb_pitch = pitch; s->rgb_stride = stride;
    return PFV_OK;
}

}  // extern "C"
