// pfv_deblock.hip -- out-of-loop deblocking of the frames that are shown: frames in device or host memory (pfv_frames_deblock*), the automatic
// strength of a q-table (pfv_deblock_strength), and the decoder session's switch (pfv_dec_set_deblock), which replaces the crop of the
// framebuffer by one k_deblock wherever a frame leaves the session.  Kernel: pfv_deblock_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

// one launch; dst: PACKED frames dst_stride bytes apart.  `g`: frame_geom(width, height, n_streams) as it comes.
static int deblock_launch(pfv_ctx *ctx, const FrameGeom &g, const SseOperand &src, uint8_t *dst, size_t dst_stride, const uint8_t strength[3])
{
    const SseOperand d = sse_operand(g, dst, PFV_FRAME_PACKED, dst_stride);   // its alignment rule is the one of 16-byte stores
    DeblockStrength st;
    for (int i = 0; i < 3; i++) st.s[i] = strength[i];
    hipLaunchKernelGGL(k_deblock, dim3(strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, src, dst, d.stride, d.vec, st);
    return launch_check(ctx, "k_deblock");
}

// slots [first, first + count) of a decoder session: the current framebuffer, filtered, as packed frames out_stride bytes apart (0: back to back)
static int dec_deblock_win(pfv_dec_session *s, int first, int count, uint8_t *frames_out_dev, size_t out_stride)
{
    pfv_ctx *ctx = s->ctx;
    FrameGeom g = s->geom;
    g.n_streams = count;
    const size_t stride = out_stride ? out_stride : (size_t)g.src_frame_bytes;
    const SseOperand src = sse_operand(g, s->fb[s->cur] + (size_t)first * (size_t)g.pad_frame_bytes, PFV_FRAME_PADDED, 0);
    return deblock_launch(ctx, g, src, frames_out_dev + (size_t)first * stride, stride, s->db_mode == PFV_DEBLOCK_FIXED ? s->db_fixed : s->db_auto);
}

extern "C" {

PFV_API int pfv_deblock_strength(const int32_t qtable[64])
{
    if (!qtable) return 0;
    const int32_t q = qtable[0] < 0 ? 0 : (qtable[0] > 65535 ? 65535 : qtable[0]);
    return std::min(kDeblockMaxS, (int)(q >> 1));
}

PFV_API int pfv_frames_deblock_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src_dev, int src_layout, size_t src_stride,
                                   uint8_t *dst_dev, size_t dst_stride, const uint8_t strength[3])
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: width/height must be positive, even and fit u16");
    if (n_streams <= 0) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: n_streams must be positive");
    if (!src_dev || !dst_dev || !strength) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: null buffer");
    if (src_layout != PFV_FRAME_PACKED && src_layout != PFV_FRAME_PADDED)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: layout must be PFV_FRAME_PACKED or PFV_FRAME_PADDED");
    for (int i = 0; i < 3; i++)
        if (strength[i] > kDeblockMaxS) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: strength above 12");
    const FrameGeom g = frame_geom(width, height, n_streams);
    const size_t src_frame = (size_t)(src_layout == PFV_FRAME_PADDED ? g.pad_frame_bytes : g.src_frame_bytes), dst_frame = (size_t)g.src_frame_bytes;
    if (src_stride && src_stride < src_frame) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: source stride below the layout's frame size");
    if (dst_stride && dst_stride < dst_frame) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: destination stride below pfv_frame_bytes");
    if ((long)g.strips_per_frame * n_streams > 0x7fffffffL) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: too many strips for one launch");
    // first frame .. end of the last one: a strip reads rows of its neighbours, so no part of the two ranges may be shared
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + (size_t)(n_streams - 1) * (src_stride ? src_stride : src_frame) + src_frame;
    const uintptr_t d0 = (uintptr_t)dst_dev, d1 = d0 + (size_t)(n_streams - 1) * (dst_stride ? dst_stride : dst_frame) + dst_frame;
    if (s0 < d1 && d0 < s1) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock_dev: source and destination overlap (in-place is not supported)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return deblock_launch(ctx, g, sse_operand(g, src_dev, src_layout, src_stride), dst_dev, dst_stride, strength);
}

PFV_API int pfv_frames_deblock(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src, uint8_t *dst, const uint8_t strength[3])
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535 || n_streams <= 0 || !src || !dst || !strength)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_deblock: bad argument (width/height positive and even, n_streams positive, no null buffer)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_deblock: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t frames = pfv_frame_bytes(width, height) * (size_t)n_streams;
    void *d_src = nullptr, *d_dst = nullptr;
    int rc;
    if ((rc = ensure_scratch(ctx, 0, frames, &d_src))) return rc;
    if ((rc = ensure_scratch(ctx, 2, frames, &d_dst))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_src, src, frames, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pfv_frames_deblock_dev(ctx, width, height, n_streams, (const uint8_t *)d_src, PFV_FRAME_PACKED, 0, (uint8_t *)d_dst, 0, strength))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_dst, frames, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

PFV_API int pfv_dec_set_deblock(pfv_dec_session *s, int mode, const uint8_t strength[3])
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    if (mode != PFV_DEBLOCK_OFF && mode != PFV_DEBLOCK_AUTO && mode != PFV_DEBLOCK_FIXED)
        return fail(s->ctx, PFV_ERR_BAD_ARG, "pfv_dec_set_deblock: mode must be PFV_DEBLOCK_OFF, _AUTO or _FIXED");
    if (mode == PFV_DEBLOCK_FIXED) {
        if (!strength) return fail(s->ctx, PFV_ERR_BAD_ARG, "pfv_dec_set_deblock: PFV_DEBLOCK_FIXED needs strengths");
        for (int i = 0; i < 3; i++)
            if (strength[i] > kDeblockMaxS) return fail(s->ctx, PFV_ERR_BAD_ARG, "pfv_dec_set_deblock: strength above 12");
        for (int i = 0; i < 3; i++) s->db_fixed[i] = strength[i];
    }
    if (mode != PFV_DEBLOCK_OFF && (s->rgb_out || s->scaled_out)) {   // the RGB / resized output then takes the filtered picture from the session's scratch: made here, never in a decode call
        const int rc = dec_present_scratch(s, "pfv_dec_set_deblock");
        if (rc) return rc;
    }
    s->db_mode = mode;
    return PFV_OK;
}

}  // extern "C"
