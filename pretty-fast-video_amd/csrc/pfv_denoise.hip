// pfv_denoise.hip -- spatio-temporal noise filter ahead of the encoder: the object that owns the streams' state and primed flags
// (pfv_denoiser), frames in device or host memory (pfv_denoiser_run_dev, pfv_frames_denoise) and the encoder session's input stage
// (pfv_enc_denoise_dev).  Kernel: pfv_denoise_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

struct pfv_denoiser {
    pfv_ctx *ctx = nullptr;
    int width = 0, height = 0, n_streams = 0;
    FrameGeom geom;                          // frame_geom(width, height, n_streams)
    uint8_t *state = nullptr;                // n_streams packed frames: each stream's previous output
    uint32_t *primed = nullptr;              // n_streams flags in device memory: non-zero once a committed run has written the stream's state
    std::vector<uint8_t> host_primed;        // what `primed` holds once the stream has run the work enqueued so far
    uint8_t ss[3] = {0, 0, 0}, st[3] = {0, 0, 0};
};

// one launch over streams [first, first + n); src / dst point at the window's first frame.  A committed run over an unprimed stream sets the
// window's flags behind the kernel.
static int denoise_launch(pfv_denoiser *dn, int first, int n, const uint8_t *src, int src_layout, size_t src_stride, uint8_t *dst, size_t dst_stride, int commit,
                          const char *who)
{
    pfv_ctx *ctx = dn->ctx;
    bool unprimed = false;
    for (int k = first; k < first + n; k++) unprimed = unprimed || !dn->host_primed[k];
    const bool prime = commit && unprimed;
    if (prime && ctx->capturing)
        return fail(ctx, PFV_ERR_STATE, std::string(who) + ": a committed run over an unprimed stream sets its flags with a memset behind the kernel -- run the first frame before pfv_graph_begin");
    FrameGeom g = dn->geom;
    g.n_streams = n;
    if ((long)g.strips_per_frame * n > 0x7fffffffL) return fail(ctx, PFV_ERR_BAD_ARG, "k_denoise: too many strips for one launch");
    const SseOperand s = sse_operand(g, src, src_layout, src_stride), d = sse_operand(g, dst, PFV_FRAME_PACKED, dst_stride);
    uint8_t *state = dn->state + (size_t)first * (size_t)g.src_frame_bytes;
    const SseOperand t = sse_operand(g, state, PFV_FRAME_PACKED, 0);
    DenoiseStrength str;
    for (int i = 0; i < 3; i++) { str.ss[i] = dn->ss[i]; str.st[i] = dn->st[i]; }
    hipLaunchKernelGGL(k_denoise, dim3(strip_blocks(g)), dim3(kThreads), 0, ctx->stream, g, s, dst, d.stride, d.vec, state, t.vec, (const uint32_t *)(dn->primed + first), str,
                       commit ? 1 : 0);
    const int rc = launch_check(ctx, "k_denoise");
    if (rc) return rc;
    if (prime) {
        HIP_TRY(ctx, hipMemsetAsync(dn->primed + first, 1, (size_t)n * sizeof(uint32_t), ctx->stream));
        for (int k = first; k < first + n; k++) dn->host_primed[k] = 1;
    }
    return PFV_OK;
}

static bool denoise_strengths_ok(const uint8_t spatial[3], const uint8_t temporal[3])
{
    for (int i = 0; i < 3; i++)
        if (spatial[i] > kDenoiseMaxS || temporal[i] > kDenoiseMaxS) return false;
    return true;
}

extern "C" {

PFV_API pfv_denoiser *pfv_denoiser_create(pfv_ctx *ctx, int width, int height, int n_streams, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    *err = PFV_OK;
    auto bad = [&](int code, const char *msg) -> pfv_denoiser * { *err = fail(ctx, code, msg); return nullptr; };
    if (!ctx) return bad(PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535)
        return bad(PFV_ERR_BAD_ARG, "pfv_denoiser_create: width/height must be positive, even and fit u16");
    if (n_streams <= 0) return bad(PFV_ERR_BAD_ARG, "pfv_denoiser_create: n_streams must be positive");
    if (ctx->capturing) return bad(PFV_ERR_STATE, "pfv_denoiser_create: the state needs an allocation, which a graph recording cannot hold");
    pfv_denoiser *dn = new pfv_denoiser;
    dn->ctx = ctx; dn->width = width; dn->height = height; dn->n_streams = n_streams;
    dn->geom = frame_geom(width, height, n_streams);
    dn->host_primed.assign((size_t)n_streams, 0);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&dn->state, (size_t)dn->geom.src_frame_bytes * (size_t)n_streams);
    if (e == hipSuccess) e = hipMalloc((void **)&dn->primed, (size_t)n_streams * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(dn->primed, 0, (size_t)n_streams * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) {
        *err = hip_fail(ctx, e, "pfv_denoiser_create");
        pfv_denoiser_destroy(dn);
        return nullptr;
    }
    return dn;
}

PFV_API void pfv_denoiser_destroy(pfv_denoiser *dn)
{
    if (!dn) return;
    (void)hipSetDevice(dn->ctx->device);
    if (dn->state || dn->primed) (void)hipStreamSynchronize(dn->ctx->stream);   // nothing enqueued reads them any more
    if (dn->state) (void)hipFree(dn->state);
    if (dn->primed) (void)hipFree(dn->primed);
    delete dn;
}

PFV_API int pfv_denoiser_set_strength(pfv_denoiser *dn, const uint8_t spatial[3], const uint8_t temporal[3])
{
    if (!dn) return fail(nullptr, PFV_ERR_BAD_ARG, "null denoiser");
    if (!spatial || !temporal) return fail(dn->ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_set_strength: null strengths");
    if (!denoise_strengths_ok(spatial, temporal)) return fail(dn->ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_set_strength: strength above 16");
    for (int i = 0; i < 3; i++) { dn->ss[i] = spatial[i]; dn->st[i] = temporal[i]; }
    return PFV_OK;
}

PFV_API int pfv_denoiser_reset(pfv_denoiser *dn, int first_stream, int n)
{
    if (!dn) return fail(nullptr, PFV_ERR_BAD_ARG, "null denoiser");
    pfv_ctx *ctx = dn->ctx;
    if (first_stream < 0 || n <= 0 || first_stream > dn->n_streams - n) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_reset: the window lies outside the denoiser's streams");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(dn->primed + first_stream, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
    for (int k = first_stream; k < first_stream + n; k++) dn->host_primed[k] = 0;
    return PFV_OK;
}

PFV_API int pfv_denoiser_run_dev(pfv_denoiser *dn, int first_stream, int n, const uint8_t *src_dev, int src_layout, size_t src_stride, uint8_t *dst_dev,
                                 size_t dst_stride, int commit)
{
    if (!dn) return fail(nullptr, PFV_ERR_BAD_ARG, "null denoiser");
    pfv_ctx *ctx = dn->ctx;
    if (first_stream < 0 || n <= 0 || first_stream > dn->n_streams - n) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_run_dev: the window lies outside the denoiser's streams");
    if (!src_dev || !dst_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_run_dev: null buffer");
    if (src_layout != PFV_FRAME_PACKED && src_layout != PFV_FRAME_PADDED)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_run_dev: layout must be PFV_FRAME_PACKED or PFV_FRAME_PADDED");
    const FrameGeom &g = dn->geom;
    const size_t src_frame = (size_t)(src_layout == PFV_FRAME_PADDED ? g.pad_frame_bytes : g.src_frame_bytes), dst_frame = (size_t)g.src_frame_bytes;
    if (src_stride && src_stride < src_frame) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_run_dev: source stride below the layout's frame size");
    if (dst_stride && dst_stride < dst_frame) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_run_dev: destination stride below pfv_frame_bytes");
    // first frame .. end of the last one: a strip reads rows of its neighbours, and the state is read and written beside both
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + (size_t)(n - 1) * (src_stride ? src_stride : src_frame) + src_frame;
    const uintptr_t d0 = (uintptr_t)dst_dev, d1 = d0 + (size_t)(n - 1) * (dst_stride ? dst_stride : dst_frame) + dst_frame;
    const uintptr_t t0 = (uintptr_t)dn->state, t1 = t0 + dst_frame * (size_t)dn->n_streams;
    if (s0 < d1 && d0 < s1) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_run_dev: source and destination overlap (in-place is not supported)");
    if ((s0 < t1 && t0 < s1) || (d0 < t1 && t0 < d1)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_denoiser_run_dev: a buffer overlaps the denoiser's state");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return denoise_launch(dn, first_stream, n, src_dev, src_layout, src_stride, dst_dev, dst_stride, commit, "pfv_denoiser_run_dev");
}

PFV_API int pfv_frames_denoise(pfv_ctx *ctx, int width, int height, int n_streams, int n_frames, const uint8_t *src, uint8_t *dst, const uint8_t spatial[3],
                               const uint8_t temporal[3])
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (n_frames <= 0 || !src || !dst || !spatial || !temporal) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_denoise: bad argument (n_frames positive, no null buffer)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_denoise: host-pointer entry points cannot be recorded");
    int rc = PFV_OK;
    pfv_denoiser *dn = pfv_denoiser_create(ctx, width, height, n_streams, &rc);
    if (!dn) return rc;
    const size_t frames = pfv_frame_bytes(width, height) * (size_t)n_streams;
    void *d_src = nullptr, *d_dst = nullptr;
    auto run = [&]() -> int {
        int r;
        if ((r = pfv_denoiser_set_strength(dn, spatial, temporal))) return r;
        if ((r = ensure_scratch(ctx, 0, frames, &d_src))) return r;
        if ((r = ensure_scratch(ctx, 2, frames, &d_dst))) return r;
        for (int f = 0; f < n_frames; f++) {   // in order on the one stream: frame f's kernel has run before frame f + 1's upload lands
            HIP_TRY(ctx, hipMemcpyAsync(d_src, src + (size_t)f * frames, frames, hipMemcpyHostToDevice, ctx->stream));
            if ((r = pfv_denoiser_run_dev(dn, 0, n_streams, (const uint8_t *)d_src, PFV_FRAME_PACKED, 0, (uint8_t *)d_dst, 0, 1))) {
                (void)hipStreamSynchronize(ctx->stream);
                return r;
            }
            HIP_TRY(ctx, hipMemcpyAsync(dst + (size_t)f * frames, d_dst, frames, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return PFV_OK;
    };
    rc = run();
    pfv_denoiser_destroy(dn);
    return rc;
}

PFV_API int pfv_enc_denoise_dev(pfv_enc_session *s, pfv_denoiser *dn, const uint8_t *frames_dev, size_t src_stride, int commit, const uint8_t **frames_dev_out)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!dn || !frames_dev || !frames_dev_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_denoise_dev: null denoiser or buffer");
    if (dn->ctx != ctx) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_denoise_dev: the denoiser belongs to another context");
    if (dn->width != s->width || dn->height != s->height || dn->n_streams != s->n_streams)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_denoise_dev: the denoiser's size or stream count is not the session's");
    const size_t fb = (size_t)s->geom.src_frame_bytes;
    if (src_stride && src_stride < fb) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_denoise_dev: source stride below pfv_frame_bytes");
    if (!src_stride) src_stride = fb;
    if (s->in_stride) return fail(ctx, PFV_ERR_STATE, "pfv_enc_denoise_dev: the session's frame buffer is packed (reset pfv_enc_session_set_frame_stride)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!s->denoise_frames) {
        if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_enc_denoise_dev: the first call allocates the session's frame buffer, which a graph recording cannot -- call once before pfv_graph_begin");
        HIP_TRY(ctx, hipMalloc((void **)&s->denoise_frames, fb * (size_t)s->n_streams));
    }
    const uint8_t *src = frames_dev + (size_t)s->win_first * src_stride;
    uint8_t *dst = s->denoise_frames + (size_t)s->win_first * fb;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)(s->win_count - 1) * src_stride + fb;
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)s->win_count * fb;
    const uintptr_t t0 = (uintptr_t)dn->state, t1 = t0 + fb * (size_t)dn->n_streams;
    if ((s0 < d1 && d0 < s1) || (s0 < t1 && t0 < s1)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_denoise_dev: the source overlaps the session's buffer or the denoiser's state");
    const int rc = denoise_launch(dn, s->win_first, s->win_count, src, PFV_FRAME_PACKED, src_stride, dst, fb, commit, "pfv_enc_denoise_dev");
    if (!rc) *frames_dev_out = s->denoise_frames;
    return rc;
}

}  // extern "C"
