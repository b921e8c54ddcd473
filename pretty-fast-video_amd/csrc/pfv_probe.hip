// pfv_probe.hip -- the i-frame size probe of an encoder session (pfv_enc_probe_iframe*): payload bytes of the window's frames as i-frames at every
// rung of the ladder, from one read of the frames.  Kernels: pfv_probe_kernels.hip.  In front of it, what all five probes' host sides share:
// the window of a launch (probe_win), the checks of their entry points (probe_dev_enter, probe_host_enter) and the packed download of a
// host-buffer call (probe_download).
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

// slots [win_first, win_first + win_count): the same launches on shifted bases (see enc_launch); geometry, grid and lane mapping are the encode
// kernels'.  ref, min_err: p-frames -- the session's current prev_frame, and min_err of every rung behind the accumulator rows (pprobe_acc)
struct ProbeWin {
    size_t first, R;
    const uint8_t *src;
    FrameGeom g;
    const uint8_t *ref;
    const float *min_err;
};
static ProbeWin probe_win(pfv_enc_session *s, const uint8_t *frames_dev, bool pframe)
{
    const size_t first = (size_t)s->win_first, R = (size_t)s->n_rungs;
    const size_t stride = s->in_stride ? s->in_stride : (size_t)s->geom.src_frame_bytes;
    const uint8_t *src = frames_dev + first * stride;
    return ProbeWin{first, R, src, enc_win_geom(s, s->win_count, src), pframe ? s->prev[s->cur] + first * (size_t)s->geom.pad_frame_bytes : nullptr,
                    pframe ? reinterpret_cast<const float *>(s->pprobe_acc + (size_t)s->n_streams * R * kPProbeAcc) : nullptr};
}

// the checks of the device-pointer entry point `who`; bufs: every buffer it requires is there
static int probe_dev_enter(pfv_enc_session *s, bool bufs, const char *who)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!bufs) return fail(ctx, PFV_ERR_BAD_ARG, std::string(who) + ": null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return PFV_OK;
}
// ... and of the host-pointer entry point `who`, which leaves the frames in the session's staging (all slots, packed)
static int probe_host_enter(pfv_enc_session *s, const uint8_t *frames, bool bufs, const char *who)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!frames || !bufs) return fail(ctx, PFV_ERR_BAD_ARG, std::string(who) + ": null buffer");
    if (!enc_full_window(s)) return fail(ctx, PFV_ERR_STATE, std::string(who) + ": the host-buffer entry points work on all slots, packed (reset the window / frame stride)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, std::string(who) + ": host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = enc_staging(s);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s->st_frames, frames, (size_t)s->geom.src_frame_bytes * s->n_streams, hipMemcpyHostToDevice, ctx->stream));
    return PFV_OK;
}

// The results of a host-buffer call, n = streams x rungs: `dev` holds sse [n][3] | ssim [n][3] (the SSIM probes) | sizes [n] | counts
// [n][kPProbeStats] (p-frames, where asked for) back to back -- the 64-bit sums first, so that every part stays aligned; one download, one
// synchronisation.  ssim_out, counts_out: null where the part is not there
static int probe_download(pfv_ctx *ctx, const void *dev, size_t n, uint64_t *sse_out, int64_t *ssim_out, uint32_t *sizes_out, uint32_t *counts_out)
{
    const size_t sum_bytes = n * 3 * sizeof(uint64_t), size_bytes = n * sizeof(uint32_t), stat_bytes = n * kPProbeStats * sizeof(uint32_t);
    const size_t sums = ssim_out ? 2 * sum_bytes : sum_bytes, bytes = sums + size_bytes + (counts_out ? stat_bytes : 0);
    std::vector<uint8_t> host(bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(sse_out, host.data(), sum_bytes);
    if (ssim_out) memcpy(ssim_out, host.data() + sum_bytes, sum_bytes);
    memcpy(sizes_out, host.data() + sums, size_bytes);
    if (counts_out) memcpy(counts_out, host.data() + sums + size_bytes, stat_bytes);
    return PFV_OK;
}

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

static int probe_launch(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev)
{
    pfv_ctx *ctx = s->ctx;
    int rc = probe_acc(s);
    if (rc) return rc;
    const ProbeWin w = probe_win(s, frames_dev, false);
    const QTab *qt = (const QTab *)s->qtab_dev;
    uint32_t *acc = s->probe_acc + w.first * w.R * kProbeAcc;
    if (use_small_grid(s->lane_mapping, w.g)) {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe<true, 16>), dim3(half_strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc);
        else hipLaunchKernelGGL((k_probe_iframe<false, 16>), dim3(half_strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc);
    } else {
        if (s->flt) hipLaunchKernelGGL((k_probe_iframe<true, 8>), dim3(strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc);
        else hipLaunchKernelGGL((k_probe_iframe<false, 8>), dim3(strip_blocks(w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, qt, s->n_rungs, acc);
    }
    hipLaunchKernelGGL(k_probe_sizes, dim3((unsigned)((size_t)s->win_count * w.R)), dim3(64), 0, ctx->stream, acc, sizes_dev + w.first * w.R,
                       stats_dev ? stats_dev + w.first * w.R * kProbeStats : (uint32_t *)nullptr);
    return launch_check(ctx, "k_probe_iframe / k_probe_sizes");
}

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

PFV_API int pfv_enc_probe_iframe_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev)
{
    int rc = probe_dev_enter(s, frames_dev && sizes_dev, "pfv_enc_probe_iframe_dev");
    return rc ? rc : probe_launch(s, frames_dev, sizes_dev, stats_dev);
}
PFV_API int pfv_enc_probe_iframe(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out)
{
    int rc = probe_host_enter(s, frames, sizes_out != nullptr, "pfv_enc_probe_iframe");
    return rc ? rc : probe_staged(s, sizes_out);
}

}  // extern "C"
