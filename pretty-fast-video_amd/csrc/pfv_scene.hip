// pfv_scene.hip -- scene-cut detection: the object that owns the streams' previous quarter planes and primed flags (pfv_scene_detector), frames
// of many streams or of one clip in device memory (pfv_scene_detector_run_dev / _run_clip_dev), host frames (pfv_frames_scene) and the pure
// host functions that turn the sums into a score and a plan of frame types (pfv_scene_score_q8, pfv_scene_plan).
// Kernels: pfv_scene_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

static_assert(sizeof(pfv_scene_stats) == 40, "k_scene_sum writes five 64-bit words per pair");

struct pfv_scene_detector {
    pfv_ctx *ctx = nullptr;
    int width = 0, height = 0, n_streams = 0, max_clip = 0;
    int cap = 0;                             // max(n_streams, max_clip): pairs of one launch group
    int radius = PFV_SCENE_RADIUS_DEFAULT;
    FrameGeom geom;                          // frame_geom(width, height, 1): the layouts' frame sizes and the luma row strides
    SceneGeom sg;
    uint8_t *state = nullptr;                // n_streams quarter planes: each stream's previous frame
    uint32_t *primed = nullptr;              // n_streams flags in device memory: non-zero once a committed run has written the stream's state
    std::vector<uint8_t> host_primed;        // what `primed` holds once the stream has run the work enqueued so far
    uint8_t *quarter = nullptr;              // cap quarter planes: the frames of the run
    uint32_t *blk = nullptr, *aux = nullptr; // cap x n_blocks: best << 16 | intra; zero | moving << 16
    int8_t *vec = nullptr;                   // cap x n_blocks x 2
};

static SceneGeom scene_geom(int w, int h)
{
    SceneGeom sg;
    sg.w = w; sg.h = h;
    sg.qw = w >> 2; sg.qh = h >> 2;
    sg.qs = (sg.qw + 7) & ~7;
    sg.nbx = sg.qw >> 3; sg.nby = sg.qh >> 3;
    sg.qbytes = (long)sg.qs * sg.qh;
    return sg;
}

// One launch group over pairs [0, n): frames at src (n of them, src_stride apart) -> quarter planes `slot0` .. of the scratch, searched against
// the state of streams first .. (clip == 0) or against the state of stream `first` and then one another (clip != 0); stats_dev [n].  With
// commit the quarter planes become the state behind the kernels, and unprimed streams of the window are primed.  ev (or nullptr): four events
// recorded around the three kernels.
static int scene_launch(pfv_scene_detector *det, int first, int n, int clip, const uint8_t *src, int layout, size_t src_stride, int commit, pfv_scene_stats *stats_dev,
                        const char *who, hipEvent_t *ev = nullptr)
{
    pfv_ctx *ctx = det->ctx;
    const int n_flags = clip ? 1 : n;
    bool unprimed = false;
    for (int k = first; k < first + n_flags; k++) unprimed = unprimed || !det->host_primed[k];
    const bool prime = commit && unprimed;
    if (prime && ctx->capturing)
        return fail(ctx, PFV_ERR_STATE, std::string(who) + ": a committed run over an unprimed stream sets its flags with a memset behind the kernels -- run the first frame before pfv_graph_begin");
    const SceneGeom &sg = det->sg;
    const size_t qb = (size_t)sg.qbytes, nb = (size_t)sg.nbx * (size_t)sg.nby;
    const int slot0 = clip ? 0 : first;      // run_dev keeps every stream's planes and maps at the stream's own index
    FrameGeom g = det->geom;
    g.n_streams = n;
    const SseOperand s = sse_operand(g, src, layout, src_stride);
    uint8_t *quarter = det->quarter + (size_t)slot0 * qb;
    const uint8_t *state = det->state + (size_t)first * qb;
    const uint32_t *primed = det->primed + first;
    uint32_t *blk = det->blk + (size_t)slot0 * nb, *aux = det->aux + (size_t)slot0 * nb;
    int8_t *vec = det->vec + (size_t)slot0 * nb * 2;
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
    if (qb) {
        const size_t lanes = (size_t)n * (size_t)sg.qh * (size_t)(sg.qs >> 2);
        hipLaunchKernelGGL(k_scene_quarter, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, sg, s, s.padded ? g.p[0].pw : g.p[0].w, n, quarter);
    }
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
    if (nb)
        hipLaunchKernelGGL(k_scene_cost, dim3((unsigned)((nb * (size_t)n + kStripsPerWG - 1) / kStripsPerWG)), dim3(kThreads), 0, ctx->stream, sg, state, (const uint8_t *)quarter, primed,
                           clip, n, det->radius, blk, vec, aux);
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[2], ctx->stream));
    hipLaunchKernelGGL(k_scene_sum, dim3((unsigned)n), dim3(kThreads), 0, ctx->stream, sg, (const uint32_t *)blk, (const uint32_t *)aux, primed, clip,
                       reinterpret_cast<unsigned long long *>(stats_dev));
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[3], ctx->stream));
    const int rc = launch_check(ctx, "k_scene_quarter / k_scene_cost / k_scene_sum");
    if (rc) return rc;
    if (!commit) return PFV_OK;
    if (qb) {
        if (clip) HIP_TRY(ctx, hipMemcpyAsync(det->state + (size_t)first * qb, quarter + (size_t)(n - 1) * qb, qb, hipMemcpyDeviceToDevice, ctx->stream));
        else HIP_TRY(ctx, hipMemcpyAsync(det->state + (size_t)first * qb, quarter, (size_t)n * qb, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (prime) {
        HIP_TRY(ctx, hipMemsetAsync(det->primed + first, 1, (size_t)n_flags * sizeof(uint32_t), ctx->stream));
        for (int k = first; k < first + n_flags; k++) det->host_primed[k] = 1;
    }
    return PFV_OK;
}

// what run_dev and run_clip_dev check alike
static int scene_run_args(pfv_scene_detector *det, int n, const uint8_t *src, int layout, size_t stride, const pfv_scene_stats *stats_dev, const char *who)
{
    pfv_ctx *ctx = det->ctx;
    if (!src || !stats_dev) return fail(ctx, PFV_ERR_BAD_ARG, std::string(who) + ": null buffer");
    if ((uintptr_t)stats_dev & 7) return fail(ctx, PFV_ERR_BAD_ARG, std::string(who) + ": stats_dev must be 8-byte aligned");
    if (layout != PFV_FRAME_PACKED && layout != PFV_FRAME_PADDED) return fail(ctx, PFV_ERR_BAD_ARG, std::string(who) + ": layout must be PFV_FRAME_PACKED or PFV_FRAME_PADDED");
    const size_t frame = (size_t)(layout == PFV_FRAME_PADDED ? det->geom.pad_frame_bytes : det->geom.src_frame_bytes);
    if (stride && stride < frame) return fail(ctx, PFV_ERR_BAD_ARG, std::string(who) + ": stride below the layout's frame size");
    if ((size_t)det->sg.nbx * (size_t)det->sg.nby * (size_t)n > 0x7fffffffUL || (size_t)det->sg.qbytes * (size_t)n > ((size_t)0x7fffffffUL << 2))
        return fail(ctx, PFV_ERR_BAD_ARG, std::string(who) + ": too many blocks for one launch");
    return PFV_OK;
}

extern "C" {

PFV_API uint32_t pfv_scene_score_q8(const pfv_scene_stats *st)
{
    if (!st || st->n_blocks == 0) return 0;
    const uint64_t den = std::max<uint64_t>(st->intra, 64ull * st->n_blocks);
    const unsigned __int128 q = (unsigned __int128)st->inter * 256 / den;   // any 64-bit inter: the product does not wrap
    return q > 65535 ? 65535u : (uint32_t)q;
}

PFV_API int pfv_scene_plan(const pfv_scene_stats *stats, int n_frames, uint32_t threshold_q8, int min_interval, int max_interval, uint8_t *types_out)
{
    if (!stats || !types_out || n_frames <= 0 || min_interval < 0 || max_interval < 0) return PFV_ERR_BAD_ARG;
    const int min_d = std::max(1, min_interval);
    int n_i = 0, last = 0;
    for (int k = 0; k < n_frames; k++) {
        const int d = k - last;
        const bool iframe = k == 0 || (max_interval > 0 && d >= max_interval) || (pfv_scene_score_q8(&stats[k]) >= threshold_q8 && d >= min_d);
        types_out[k] = iframe ? 1 : 2;
        if (iframe) { last = k; n_i++; }
    }
    return n_i;
}

PFV_API pfv_scene_detector *pfv_scene_detector_create(pfv_ctx *ctx, int width, int height, int n_streams, int max_clip_frames, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    *err = PFV_OK;
    auto bad = [&](int code, const char *msg) -> pfv_scene_detector * { *err = fail(ctx, code, msg); return nullptr; };
    if (!ctx) return bad(PFV_ERR_BAD_ARG, "null ctx");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || width > 65535 || height > 65535)
        return bad(PFV_ERR_BAD_ARG, "pfv_scene_detector_create: width/height must be positive, even and fit u16");
    if (n_streams <= 0 || max_clip_frames < 0) return bad(PFV_ERR_BAD_ARG, "pfv_scene_detector_create: n_streams must be positive, max_clip_frames not negative");
    if (ctx->capturing) return bad(PFV_ERR_STATE, "pfv_scene_detector_create: the state needs an allocation, which a graph recording cannot hold");
    pfv_scene_detector *det = new pfv_scene_detector;
    det->ctx = ctx; det->width = width; det->height = height; det->n_streams = n_streams; det->max_clip = max_clip_frames;
    det->cap = std::max(n_streams, max_clip_frames);
    det->geom = frame_geom(width, height, 1);
    det->sg = scene_geom(width, height);
    det->host_primed.assign((size_t)n_streams, 0);
    const size_t qb = (size_t)det->sg.qbytes, nb = (size_t)det->sg.nbx * (size_t)det->sg.nby, cap = (size_t)det->cap;
    auto at_least = [](size_t b) { return b ? b : (size_t)16; };
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&det->state, at_least(qb * (size_t)n_streams));
    if (e == hipSuccess) e = hipMalloc((void **)&det->primed, (size_t)n_streams * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&det->quarter, at_least(qb * cap));
    if (e == hipSuccess) e = hipMalloc((void **)&det->blk, at_least(nb * cap * sizeof(uint32_t)));
    if (e == hipSuccess) e = hipMalloc((void **)&det->aux, at_least(nb * cap * sizeof(uint32_t)));
    if (e == hipSuccess) e = hipMalloc((void **)&det->vec, at_least(nb * cap * 2));
    if (e == hipSuccess) e = hipMemsetAsync(det->primed, 0, (size_t)n_streams * sizeof(uint32_t), ctx->stream);
    // the maps of a run that has not happened read as zeros
    if (e == hipSuccess) e = hipMemsetAsync(det->blk, 0, at_least(nb * cap * sizeof(uint32_t)), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(det->vec, 0, at_least(nb * cap * 2), ctx->stream);
    if (e != hipSuccess) {
        *err = hip_fail(ctx, e, "pfv_scene_detector_create");
        pfv_scene_detector_destroy(det);
        return nullptr;
    }
    return det;
}

PFV_API void pfv_scene_detector_destroy(pfv_scene_detector *det)
{
    if (!det) return;
    (void)hipSetDevice(det->ctx->device);
    (void)hipStreamSynchronize(det->ctx->stream);   // nothing enqueued reads the buffers any more
    void *bufs[] = {det->state, det->primed, det->quarter, det->blk, det->aux, det->vec};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete det;
}

PFV_API int pfv_scene_detector_set_radius(pfv_scene_detector *det, int radius)
{
    if (!det) return fail(nullptr, PFV_ERR_BAD_ARG, "null detector");
    if (radius < 0 || radius > kSceneMaxR) return fail(det->ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_set_radius: the radius is 0 .. 7 quarter samples");
    det->radius = radius;
    return PFV_OK;
}

PFV_API int pfv_scene_detector_reset(pfv_scene_detector *det, int first_stream, int n)
{
    if (!det) return fail(nullptr, PFV_ERR_BAD_ARG, "null detector");
    pfv_ctx *ctx = det->ctx;
    if (first_stream < 0 || n <= 0 || first_stream > det->n_streams - n) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_reset: the window lies outside the detector's streams");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(det->primed + first_stream, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
    for (int k = first_stream; k < first_stream + n; k++) det->host_primed[k] = 0;
    return PFV_OK;
}

PFV_API int pfv_scene_detector_run_dev(pfv_scene_detector *det, int first_stream, int n, const uint8_t *src_dev, int src_layout, size_t src_stride, int commit,
                                       pfv_scene_stats *stats_dev)
{
    if (!det) return fail(nullptr, PFV_ERR_BAD_ARG, "null detector");
    pfv_ctx *ctx = det->ctx;
    if (first_stream < 0 || n <= 0 || first_stream > det->n_streams - n) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_run_dev: the window lies outside the detector's streams");
    int rc = scene_run_args(det, n, src_dev, src_layout, src_stride, stats_dev, "pfv_scene_detector_run_dev");
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return scene_launch(det, first_stream, n, 0, src_dev, src_layout, src_stride, commit, stats_dev, "pfv_scene_detector_run_dev");
}

PFV_API int pfv_scene_detector_run_clip_dev(pfv_scene_detector *det, int stream, int n_frames, const uint8_t *frames_dev, int layout, size_t stride, int commit,
                                            pfv_scene_stats *stats_dev)
{
    if (!det) return fail(nullptr, PFV_ERR_BAD_ARG, "null detector");
    pfv_ctx *ctx = det->ctx;
    if (stream < 0 || stream >= det->n_streams) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_run_clip_dev: no such stream");
    if (n_frames <= 0 || n_frames > det->max_clip) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_run_clip_dev: n_frames must be 1 .. max_clip_frames");
    int rc = scene_run_args(det, n_frames, frames_dev, layout, stride, stats_dev, "pfv_scene_detector_run_clip_dev");
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return scene_launch(det, stream, n_frames, 1, frames_dev, layout, stride, commit, stats_dev, "pfv_scene_detector_run_clip_dev");
}

PFV_API int pfv_scene_detector_run_timed_dev(pfv_scene_detector *det, int first, int n, int clip, const uint8_t *src_dev, int layout, size_t stride,
                                             pfv_scene_stats *stats_dev, float ms_out[3])
{
    if (!det) return fail(nullptr, PFV_ERR_BAD_ARG, "null detector");
    pfv_ctx *ctx = det->ctx;
    if (!ms_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_run_timed_dev: null buffer");
    if (clip ? (first < 0 || first >= det->n_streams || n <= 0 || n > det->max_clip) : (first < 0 || n <= 0 || first > det->n_streams - n))
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_run_timed_dev: the window lies outside the detector's streams or clip frames");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_scene_detector_run_timed_dev: a timed run synchronises and cannot be recorded");
    int rc = scene_run_args(det, n, src_dev, layout, stride, stats_dev, "pfv_scene_detector_run_timed_dev");
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipEvent_t ev[4] = {};
    auto drop = [&]() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); };
    for (hipEvent_t &e : ev)
        if (hipEventCreateWithFlags(&e, hipEventDefault) != hipSuccess) { drop(); return fail(ctx, PFV_ERR_HIP, "pfv_scene_detector_run_timed_dev: hipEventCreate"); }
    rc = scene_launch(det, first, n, clip ? 1 : 0, src_dev, layout, stride, 0, stats_dev, "pfv_scene_detector_run_timed_dev", ev);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, PFV_ERR_HIP, "pfv_scene_detector_run_timed_dev: hipStreamSynchronize");
    for (int k = 0; k < 3 && !rc; k++)
        if (hipEventElapsedTime(&ms_out[k], ev[k], ev[k + 1]) != hipSuccess) rc = fail(ctx, PFV_ERR_HIP, "pfv_scene_detector_run_timed_dev: hipEventElapsedTime");
    drop();
    return rc;
}

PFV_API int pfv_scene_detector_maps(pfv_scene_detector *det, int first, int n, uint32_t *blk_out, int8_t *vec_out)
{
    if (!det) return fail(nullptr, PFV_ERR_BAD_ARG, "null detector");
    pfv_ctx *ctx = det->ctx;
    if (first < 0 || n <= 0 || first > det->cap - n) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_maps: the window lies outside the detector's entries");
    if (!blk_out && !vec_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scene_detector_maps: null buffers");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_scene_detector_maps: host-pointer entry points cannot be recorded");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)det->sg.nbx * (size_t)det->sg.nby;
    if (nb && blk_out) HIP_TRY(ctx, hipMemcpyAsync(blk_out, det->blk + (size_t)first * nb, (size_t)n * nb * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (nb && vec_out) HIP_TRY(ctx, hipMemcpyAsync(vec_out, det->vec + (size_t)first * nb * 2, (size_t)n * nb * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFV_OK;
}

PFV_API int pfv_frames_scene(pfv_ctx *ctx, int width, int height, int n_streams, int n_frames, const uint8_t *frames, int radius, pfv_scene_stats *stats_out)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (n_frames <= 0 || !frames || !stats_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_scene: bad argument (n_frames positive, no null buffer)");
    if (radius < 0 || radius > kSceneMaxR) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_scene: the radius is 0 .. 7 quarter samples");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_scene: host-pointer entry points cannot be recorded");
    int rc = PFV_OK;
    pfv_scene_detector *det = pfv_scene_detector_create(ctx, width, height, n_streams, 0, &rc);
    if (!det) return rc;
    const size_t group = pfv_frame_bytes(width, height) * (size_t)n_streams, n_stats = (size_t)n_frames * (size_t)n_streams;
    void *d_src = nullptr, *d_stats = nullptr;
    auto run = [&]() -> int {
        int r;
        if ((r = pfv_scene_detector_set_radius(det, radius))) return r;
        if ((r = ensure_scratch(ctx, 0, group, &d_src))) return r;
        if ((r = ensure_scratch(ctx, 2, n_stats * sizeof(pfv_scene_stats), &d_stats))) return r;
        for (int f = 0; f < n_frames; f++) {   // in order on the one stream: frame f's kernels have run before frame f + 1's upload lands
            HIP_TRY(ctx, hipMemcpyAsync(d_src, frames + (size_t)f * group, group, hipMemcpyHostToDevice, ctx->stream));
            if ((r = pfv_scene_detector_run_dev(det, 0, n_streams, (const uint8_t *)d_src, PFV_FRAME_PACKED, 0, 1, (pfv_scene_stats *)d_stats + (size_t)f * (size_t)n_streams))) {
                (void)hipStreamSynchronize(ctx->stream);
                return r;
            }
        }
        HIP_TRY(ctx, hipMemcpyAsync(stats_out, d_stats, n_stats * sizeof(pfv_scene_stats), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return PFV_OK;
    };
    rc = run();
    pfv_scene_detector_destroy(det);
    return rc;
}

}  // extern "C"
