// pfv_pprobe.hip -- the p-frame size probe of an encoder session (pfv_enc_probe_pframe*): payload bytes of the window's frames as p-frames against
// the session's current prev_frame at every rung of the ladder, from one search and one forward transform.  Kernels: pfv_pprobe_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

// the kernels' accumulator and, behind it, min_err of every rung: made, cleared and filled by the first call; the rows are left clear by every
// k_pprobe_sizes
static int pprobe_acc(pfv_enc_session *s)
{
    pfv_ctx *ctx = s->ctx;
    if (s->pprobe_acc) return PFV_OK;
    if (ctx->capturing)
        return fail(ctx, PFV_ERR_STATE, "pfv_enc_probe_pframe_dev: the accumulator needs an allocation, which a graph recording cannot hold -- call once before pfv_graph_begin");
    const size_t words = (size_t)s->n_streams * (size_t)s->n_rungs * kPProbeAcc;
    float min_err[kMaxRungs] = {0.0f};
    for (int r = 0; r < s->n_rungs; r++) min_err[r] = s->px_err[r] * s->px_err[r] * 256.0f;   // src/common.rs:209, as enc_launch forms it
    HIP_TRY(ctx, hipMalloc((void **)&s->pprobe_acc, (words + kMaxRungs) * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(s->pprobe_acc, 0, words * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->pprobe_acc + words, min_err, sizeof min_err, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // min_err lives on this stack frame
    if (e != hipSuccess) {
        (void)hipFree(s->pprobe_acc);
        s->pprobe_acc = nullptr;
        return hip_fail(ctx, e, "pfv_enc_probe_pframe_dev");
    }
    return PFV_OK;
}

static int pprobe_launch(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev)
{
    pfv_ctx *ctx = s->ctx;
    int rc = pprobe_acc(s);
    if (rc) return rc;
    const ProbeWin w = probe_win(s, frames_dev, true);
    const QTab *qt = (const QTab *)s->qtab_dev;
    uint32_t *acc = s->pprobe_acc + w.first * w.R * kPProbeAcc;
    if (s->flt) hipLaunchKernelGGL(k_probe_pframe<true>, dim3(penc_blocks(ctx, w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, w.ref, qt, s->n_rungs, w.min_err, -2, acc);
    else hipLaunchKernelGGL(k_probe_pframe<false>, dim3(penc_blocks(ctx, w.g)), dim3(kThreads), 0, ctx->stream, w.g, w.src, w.ref, qt, s->n_rungs, w.min_err, -2, acc);
    hipLaunchKernelGGL(k_pprobe_sizes, dim3((unsigned)((size_t)s->win_count * w.R)), dim3(64), 0, ctx->stream, acc, sizes_dev + w.first * w.R,
                       stats_dev ? stats_dev + w.first * w.R * kPProbeStats : (uint32_t *)nullptr);
    return launch_check(ctx, "k_probe_pframe / k_pprobe_sizes");
}

// the frames in the session's staging (all slots, packed) -> sizes_out [n_streams][n_rungs] and, where asked for, stats_out
// [n_streams][n_rungs][kPProbeStats]; synchronises
static int pprobe_staged(pfv_enc_session *s, uint32_t *sizes_out, uint32_t *stats_out = nullptr)
{
    pfv_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->n_streams * (size_t)s->n_rungs;
    if (!s->pprobe_out) HIP_TRY(ctx, hipMalloc((void **)&s->pprobe_out, n * (1 + kPProbeStats) * sizeof(uint32_t)));
    int rc = pprobe_launch(s, s->st_frames, s->pprobe_out, stats_out ? s->pprobe_out + n : nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIP_TRY(ctx, hipMemcpyAsync(sizes_out, s->pprobe_out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (stats_out) HIP_TRY(ctx, hipMemcpyAsync(stats_out, s->pprobe_out + n, n * kPProbeStats * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

extern "C" {

PFV_API int pfv_enc_probe_pframe_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev)
{
    if (int rf = enc_pframe_probe_refused(s, "pfv_enc_probe_pframe_dev")) return rf;
    int rc = probe_dev_enter(s, frames_dev && sizes_dev, "pfv_enc_probe_pframe_dev");
    return rc ? rc : pprobe_launch(s, frames_dev, sizes_dev, stats_dev);
}
PFV_API int pfv_enc_probe_pframe(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out)
{
    if (int rf = enc_pframe_probe_refused(s, "pfv_enc_probe_pframe")) return rf;
    int rc = probe_host_enter(s, frames, sizes_out != nullptr, "pfv_enc_probe_pframe");
    return rc ? rc : pprobe_staged(s, sizes_out);
}

}  // extern "C"
