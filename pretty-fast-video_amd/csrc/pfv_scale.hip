// pfv_scale.hip -- frame resize: the filter tables (pfv_scale_taps, pfv_scale_table: host only), the plan object that holds a size pair's four
// tables on the device (pfv_scaler), frames in device or host memory (pfv_scaler_run_dev, pfv_frames_scale).  Kernel: pfv_scale_kernels.hip.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.

static bool scale_kind_ok(int kind) { return kind == PFV_SCALE_BILINEAR || kind == PFV_SCALE_BICUBIC || kind == PFV_SCALE_LANCZOS3; }

// the kernel K(t) of a kind, in IEEE double, every operation rounded on its own
static double scale_weight(int kind, double t)
{
#pragma clang fp contract(off)
    const double a = fabs(t);
    if (kind == PFV_SCALE_BILINEAR) return a < 1.0 ? 1.0 - a : 0.0;
    if (kind == PFV_SCALE_BICUBIC) {
        if (a < 1.0) return (1.5 * a - 2.5) * a * a + 1.0;
        if (a < 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
        return 0.0;
    }
    if (a >= 3.0) return 0.0;
    if (a == 0.0) return 1.0;
    const double x = M_PI * a, y = x / 3.0;
    return (sin(x) / x) * (sin(y) / y);
}

struct pfv_scaler {
    pfv_ctx *ctx = nullptr;
    int sw = 0, sh = 0, dw = 0, dh = 0, kind = 0;
    void *tables = nullptr;                 // one allocation: luma x, luma y, chroma x, chroma y -- each first[] then coef[]
    ScaleAxis axis[4];                      // device pointers into `tables`
};

static bool scale_dims_ok(int w, int h) { return w > 0 && h > 0 && !(w & 1) && !(h & 1) && w <= 65535 && h <= 65535; }

extern "C" {

PFV_API int pfv_scale_taps(int kind, int n_src, int n_dst)
{
    if (!scale_kind_ok(kind) || n_src <= 0 || n_dst <= 0 || n_src > 65535 || n_dst > 65535 || n_src > kScaleMaxRatio * n_dst) return 0;
    const int S = kind + 1;
    return n_src > n_dst ? 2 * ((S * n_src + n_dst - 1) / n_dst) : 2 * S;
}

PFV_API int pfv_scale_table(int kind, int n_src, int n_dst, int32_t *first, int16_t *coef)
{
#pragma clang fp contract(off)
    const int T = pfv_scale_taps(kind, n_src, n_dst);
    if (!T) return fail(nullptr, PFV_ERR_BAD_ARG, "pfv_scale_table: a kind that does not exist, a size outside 1 .. 65535 or a reduction beyond 8");
    if (!first || !coef) return fail(nullptr, PFV_ERR_BAD_ARG, "pfv_scale_table: null buffer");
    const int S = kind + 1;
    const int64_t m = std::max(n_src, n_dst);
    const double f = n_src > n_dst ? (double)n_src / (double)n_dst : 1.0;
    double w[kScaleMaxTaps];
    for (int o = 0; o < n_dst; o++) {
        const int64_t num = (int64_t)(2 * o + 1) * n_src - n_dst, a = num - 2 * S * m, b = 2 * (int64_t)n_dst;
        const int64_t left = (a >= 0 ? a / b : -((-a + b - 1) / b)) + 1;        // floor toward minus infinity
        const double c = (double)num / (2.0 * (double)n_dst);
        double sum = 0.0;
        for (int k = 0; k < T; k++) {
            w[k] = scale_weight(kind, ((double)(left + k) - c) / f);
            sum = sum + w[k];
        }
        int32_t q[kScaleMaxTaps];
        int total = 0, big = 0, mag = 0;
        for (int k = 0; k < T; k++) {
            q[k] = (int32_t)rint(w[k] / sum * 16384.0);
            total += q[k];
            if (abs(q[k]) > abs(q[big])) big = k;
        }
        q[big] += 16384 - total;
        for (int k = 0; k < T; k++) {
            mag += abs(q[k]);
            if (q[k] < -32768 || q[k] > 32767) return fail(nullptr, PFV_ERR_BAD_ARG, "pfv_scale_table: a coefficient leaves int16");
            coef[(size_t)o * T + k] = (int16_t)q[k];
        }
        if (mag >= 65536) return fail(nullptr, PFV_ERR_BAD_ARG, "pfv_scale_table: a row's absolute sum reaches 65536");
        first[o] = (int32_t)left;
    }
    return PFV_OK;
}

PFV_API pfv_scaler *pfv_scaler_create(pfv_ctx *ctx, int sw, int sh, int dw, int dh, int kind, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    *err = PFV_OK;
    auto bad = [&](int code, const char *msg) -> pfv_scaler * { *err = fail(ctx, code, msg); return nullptr; };
    if (!ctx) return bad(PFV_ERR_BAD_ARG, "null ctx");
    if (!scale_kind_ok(kind)) return bad(PFV_ERR_BAD_ARG, "pfv_scaler_create: kind must be PFV_SCALE_BILINEAR, _BICUBIC or _LANCZOS3");
    if (!scale_dims_ok(sw, sh) || !scale_dims_ok(dw, dh)) return bad(PFV_ERR_BAD_ARG, "pfv_scaler_create: widths and heights must be positive, even and fit u16");
    if (sw > kScaleMaxRatio * dw || sh > kScaleMaxRatio * dh) return bad(PFV_ERR_BAD_ARG, "pfv_scaler_create: a reduction beyond 8 on one axis -- chain two scalers");
    if (ctx->capturing) return bad(PFV_ERR_STATE, "pfv_scaler_create: the tables need an allocation and an upload, which a graph recording cannot hold");
    const int ns[4] = {sw, sh, sw / 2, sh / 2}, nd[4] = {dw, dh, dw / 2, dh / 2};
    size_t at[4], bytes = 0;
    int taps[4];
    for (int i = 0; i < 4; i++) {
        taps[i] = pfv_scale_taps(kind, ns[i], nd[i]);
        at[i] = bytes;
        bytes += ((size_t)nd[i] * 4 + (size_t)nd[i] * taps[i] * 2 + 15) & ~(size_t)15;
    }
    std::vector<uint8_t> host(bytes, 0);
    for (int i = 0; i < 4; i++) {
        const int rc = pfv_scale_table(kind, ns[i], nd[i], (int32_t *)(host.data() + at[i]), (int16_t *)(host.data() + at[i] + (size_t)nd[i] * 4));
        if (rc) { *err = rc; if (ctx) ctx->err = g_tls_err; return nullptr; }
    }
    pfv_scaler *sc = new pfv_scaler;
    sc->ctx = ctx; sc->sw = sw; sc->sh = sh; sc->dw = dw; sc->dh = dh; sc->kind = kind;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&sc->tables, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(sc->tables, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // `host` goes away
    if (e != hipSuccess) {
        *err = hip_fail(ctx, e, "pfv_scaler_create");
        if (sc->tables) (void)hipFree(sc->tables);
        delete sc;
        return nullptr;
    }
    for (int i = 0; i < 4; i++) {
        uint8_t *t = (uint8_t *)sc->tables + at[i];
        sc->axis[i] = ScaleAxis{(const int32_t *)t, (const int16_t *)(t + (size_t)nd[i] * 4), taps[i], ns[i], nd[i]};
    }
    return sc;
}

PFV_API void pfv_scaler_destroy(pfv_scaler *sc)
{
    if (!sc) return;
    if (sc->tables) {
        (void)hipSetDevice(sc->ctx->device);
        (void)hipFree(sc->tables);
    }
    delete sc;
}

}  // extern "C"

// one launch.  The wide forms need, per plane, every row to start on a 4-byte boundary: base, stream stride, plane offset and row pitch.
static int scale_launch(pfv_scaler *sc, int n_streams, const uint8_t *src, int src_layout, size_t src_stride, uint8_t *dst, size_t dst_stride)
{
    pfv_ctx *ctx = sc->ctx;
    if (n_streams > 65535) return fail(ctx, PFV_ERR_BAD_ARG, "k_scale: too many streams for one launch");
    const FrameGeom gs = frame_geom(sc->sw, sc->sh, n_streams), gd = frame_geom(sc->dw, sc->dh, n_streams);
    const bool padded = src_layout == PFV_FRAME_PADDED;
    ScaleArgs a;
    memset(&a, 0, sizeof a);
    a.src = src; a.dst = dst;
    a.src_stride = (long)src_stride; a.dst_stride = (long)dst_stride;
    int tiles = 0;
    for (int i = 0; i < 3; i++) {
        ScalePlane &p = a.p[i];
        p.x = sc->axis[i ? 2 : 0];
        p.y = sc->axis[i ? 3 : 1];
        p.src_off = padded ? gs.p[i].pad_off : gs.p[i].src_off;
        p.src_pitch = padded ? gs.p[i].pw : gs.p[i].w;
        p.dst_off = gd.p[i].src_off;
        p.tiles_x = (p.x.n_dst + kScaleTW - 1) / kScaleTW;
        p.tile0 = tiles;
        tiles += p.tiles_x * ((p.y.n_dst + kScaleTH - 1) / kScaleTH);
        if (((uintptr_t)src & 3) == 0 && src_stride % 4 == 0 && p.src_off % 4 == 0 && p.src_pitch % 4 == 0) a.wide_src |= 1 << i;
        if (((uintptr_t)dst & 3) == 0 && dst_stride % 4 == 0 && p.dst_off % 4 == 0 && p.x.n_dst % 4 == 0) a.wide_dst |= 1 << i;
    }
    hipLaunchKernelGGL(k_scale, dim3((unsigned)tiles, (unsigned)n_streams), dim3(kScaleThreads), 0, ctx->stream, a);
    return launch_check(ctx, "k_scale");
}

extern "C" {

PFV_API int pfv_scaler_run_dev(pfv_scaler *sc, int n_streams, const uint8_t *src_dev, int src_layout, size_t src_stride, uint8_t *dst_dev, size_t dst_stride)
{
    if (!sc) return fail(nullptr, PFV_ERR_BAD_ARG, "null scaler");
    pfv_ctx *ctx = sc->ctx;
    if (n_streams <= 0) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scaler_run_dev: n_streams must be positive");
    if (!src_dev || !dst_dev) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scaler_run_dev: null buffer");
    if (src_layout != PFV_FRAME_PACKED && src_layout != PFV_FRAME_PADDED)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scaler_run_dev: layout must be PFV_FRAME_PACKED or PFV_FRAME_PADDED");
    const size_t src_frame = src_layout == PFV_FRAME_PADDED ? pfv_padded_frame_bytes(sc->sw, sc->sh) : pfv_frame_bytes(sc->sw, sc->sh);
    const size_t dst_frame = pfv_frame_bytes(sc->dw, sc->dh);
    if (src_stride && src_stride < src_frame) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scaler_run_dev: source stride below the layout's frame size");
    if (dst_stride && dst_stride < dst_frame) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scaler_run_dev: destination stride below pfv_frame_bytes");
    if (!src_stride) src_stride = src_frame;
    if (!dst_stride) dst_stride = dst_frame;
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + (size_t)(n_streams - 1) * src_stride + src_frame;
    const uintptr_t d0 = (uintptr_t)dst_dev, d1 = d0 + (size_t)(n_streams - 1) * dst_stride + dst_frame;
    if (s0 < d1 && d0 < s1) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_scaler_run_dev: source and destination overlap");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return scale_launch(sc, n_streams, src_dev, src_layout, src_stride, dst_dev, dst_stride);
}

PFV_API int pfv_frames_scale(pfv_ctx *ctx, int sw, int sh, int dw, int dh, int n_streams, const uint8_t *src, uint8_t *dst, int kind)
{
    if (!ctx) return fail(nullptr, PFV_ERR_BAD_ARG, "null ctx");
    if (n_streams <= 0 || !src || !dst) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_frames_scale: bad argument (n_streams positive, no null buffer)");
    if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_frames_scale: host-pointer entry points cannot be recorded");
    int rc = PFV_OK;
    pfv_scaler *sc = pfv_scaler_create(ctx, sw, sh, dw, dh, kind, &rc);
    if (!sc) return rc;
    const size_t in = pfv_frame_bytes(sw, sh) * (size_t)n_streams, out = pfv_frame_bytes(dw, dh) * (size_t)n_streams;
    void *d_src = nullptr, *d_dst = nullptr;
    auto run = [&]() -> int {
        int r;
        if ((r = ensure_scratch(ctx, 0, in, &d_src))) return r;
        if ((r = ensure_scratch(ctx, 2, out, &d_dst))) return r;
        HIP_TRY(ctx, hipMemcpyAsync(d_src, src, in, hipMemcpyHostToDevice, ctx->stream));
        if ((r = pfv_scaler_run_dev(sc, n_streams, (const uint8_t *)d_src, PFV_FRAME_PACKED, 0, (uint8_t *)d_dst, 0))) {
            (void)hipStreamSynchronize(ctx->stream);
            return r;
        }
        HIP_TRY(ctx, hipMemcpyAsync(dst, d_dst, out, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return PFV_OK;
    };
    rc = run();
    pfv_scaler_destroy(sc);
    return rc;
}

}  // extern "C"

// ---- the sessions' share
extern "C" {

PFV_API int pfv_dec_set_output_scaled_dev(pfv_dec_session *s, pfv_scaler *sc, uint8_t *dst_dev, size_t stride)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    if (!dst_dev) {
        s->scaled_out = nullptr; s->scaled_sc = nullptr;
        return PFV_OK;
    }
    pfv_ctx *ctx = s->ctx;
    if (!sc) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_set_output_scaled_dev: null scaler");
    if (sc->ctx != ctx) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_set_output_scaled_dev: the scaler belongs to another context");
    if (sc->sw != s->width || sc->sh != s->height) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_set_output_scaled_dev: the scaler's source size is not the session's");
    const size_t fb = pfv_frame_bytes(sc->dw, sc->dh);
    if (stride && stride < fb) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_dec_set_output_scaled_dev: stride below pfv_frame_bytes of the destination size");
    int rc;
    if (s->db_mode && (rc = dec_present_scratch(s, "pfv_dec_set_output_scaled_dev"))) return rc;
    s->scaled_sc = sc; s->scaled_out = dst_dev; s->scaled_stride = stride ? stride : fb;
    return PFV_OK;
}

PFV_API int pfv_enc_scale_dev(pfv_enc_session *s, pfv_scaler *sc, const uint8_t *frames_dev, size_t src_stride, const uint8_t **frames_dev_out)
{
    if (!s) return fail(nullptr, PFV_ERR_BAD_ARG, "null session");
    pfv_ctx *ctx = s->ctx;
    if (!sc || !frames_dev || !frames_dev_out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_scale_dev: null scaler or buffer");
    if (sc->ctx != ctx) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_scale_dev: the scaler belongs to another context");
    if (sc->dw != s->width || sc->dh != s->height) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_scale_dev: the scaler's destination size is not the session's");
    const size_t sfb = pfv_frame_bytes(sc->sw, sc->sh), fb = (size_t)s->geom.src_frame_bytes;
    if (src_stride && src_stride < sfb) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_enc_scale_dev: source stride below pfv_frame_bytes of the source size");
    if (!src_stride) src_stride = sfb;
    if (s->in_stride) return fail(ctx, PFV_ERR_STATE, "pfv_enc_scale_dev: the session's frame buffer is packed (reset pfv_enc_session_set_frame_stride; GOP-batched frames use the source stride)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!s->scale_frames) {
        if (ctx->capturing) return fail(ctx, PFV_ERR_STATE, "pfv_enc_scale_dev: the first call allocates the session's frame buffer, which a graph recording cannot -- call once before pfv_graph_begin");
        HIP_TRY(ctx, hipMalloc((void **)&s->scale_frames, fb * (size_t)s->n_streams));
    }
    *frames_dev_out = s->scale_frames;
    return scale_launch(sc, s->win_count, frames_dev + (size_t)s->win_first * src_stride, PFV_FRAME_PACKED, src_stride, s->scale_frames + (size_t)s->win_first * fb, fb);
}

}  // extern "C"
