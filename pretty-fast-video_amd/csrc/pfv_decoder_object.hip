// pfv_decoder_object.hip -- payload serialisers / parsers on their own, and pfv_decoder (dec::Decoder<R>) with its look-ahead machinery.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.
extern "C" {

// payload serialisers alone (for tests: product vs oracle on identical coefficient input)
PFV_API size_t pfv_serialize_iframe_payload(const int16_t *coef, int total_blocks, uint8_t *out, size_t cap)
{
    std::vector<uint8_t> p;
    if (!coef || total_blocks <= 0 || !serialize_iframe(p, coef, total_blocks)) return 0;
    if (out && p.size() <= cap) memcpy(out, p.data(), p.size());
    return p.size();
}
PFV_API size_t pfv_serialize_pframe_payload(const int8_t *mv, const uint8_t *has_coef, const int16_t *coef, int total_blocks,
                                            uint8_t *out, size_t cap)
{
    std::vector<uint8_t> p;
    if (!mv || !has_coef || !coef || total_blocks <= 0 || !serialize_pframe(p, mv, has_coef, coef, total_blocks)) return 0;
    if (out && p.size() <= cap) memcpy(out, p.data(), p.size());
    return p.size();
}

// payload parsers alone (decode_iframe / decode_pframe up to the plane decode, src/dec.rs:226-296, 328-417); host only.
// coef_out: [total_blocks][256], zero-filled first.  Returns PFV_OK, PFV_ERR_FORMAT or PFV_ERR_IO.
PFV_API int pfv_parse_iframe_payload(const uint8_t *payload, size_t len, int total_blocks, int n_qtables, int16_t *coef_out,
                                     uint8_t qidx_out[3])
{
    if (!payload || !coef_out || !qidx_out || total_blocks <= 0) return fail(nullptr, PFV_ERR_BAD_ARG, "pfv_parse_iframe_payload: bad argument");
    int rc = parse_iframe(payload, len, total_blocks, n_qtables, coef_out, qidx_out);
    return rc ? fail(nullptr, rc, "malformed packet payload") : PFV_OK;
}
PFV_API int pfv_parse_pframe_payload(const uint8_t *payload, size_t len, int total_blocks, int n_qtables, int8_t *mv_out,
                                     uint8_t *has_coef_out, int16_t *coef_out, uint8_t qidx_out[3])
{
    if (!payload || !mv_out || !has_coef_out || !coef_out || !qidx_out || total_blocks <= 0)
        return fail(nullptr, PFV_ERR_BAD_ARG, "pfv_parse_pframe_payload: bad argument");
    int rc = parse_pframe(payload, len, total_blocks, n_qtables, mv_out, has_coef_out, coef_out, qidx_out);
    return rc ? fail(nullptr, rc, "malformed packet payload") : PFV_OK;
}
// The sparse form the stream decoder uploads: up to `cap` (flat index, value) pairs; *n_out = pairs written.  Returns 1 when
// the list would overflow (the caller then parses the dense form).
PFV_API int pfv_parse_payload_sparse(int is_pframe, const uint8_t *payload, size_t len, int total_blocks, int n_qtables,
                                     int8_t *mv_out, uint8_t *has_coef_out, uint32_t *idx_out, int16_t *val_out, size_t cap,
                                     size_t *n_out, uint8_t qidx_out[3])
{
    if (!payload || !idx_out || !val_out || !n_out || !qidx_out || total_blocks <= 0 || (is_pframe && (!mv_out || !has_coef_out)))
        return fail(nullptr, PFV_ERR_BAD_ARG, "pfv_parse_payload_sparse: bad argument");
    SparseSink sink{idx_out, val_out, cap};
    int rc = parse_frame_to(is_pframe ? 2 : 1, payload, len, total_blocks, n_qtables, mv_out, has_coef_out, sink, qidx_out);
    *n_out = sink.n;
    if (rc == kSinkFull) return 1;
    return rc ? fail(nullptr, rc, "malformed packet payload") : PFV_OK;
}

// Decoder::new (src/dec.rs:38-134).  `data` must stay valid for the decoder's lifetime (R: Read + Seek).
PFV_API int pfv_decoder_create(pfv_ctx *ctx, const uint8_t *data, size_t len, pfv_decoder **out)
{
    if (!ctx || !data || !out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_decoder_create: bad argument");
    *out = nullptr;
    PfvHeader hd;
    int rc = read_header(ctx, data, len, hd);
    if (rc) return rc;
    const int w = hd.width, h = hd.height;
    pfv_dec_session *hot = nullptr;
    if ((rc = pfv_dec_session_create(ctx, w, h, hd.q.data(), hd.n_qtables, 1, &hot))) return rc;
    pfv_decoder *d = new pfv_decoder();
    d->ctx = ctx; d->hot = hot; d->data = data; d->len = len;
    d->pos = d->reset_pos = d->scan_pos = hd.len;
    d->width = w; d->height = h; d->framerate = hd.framerate; d->n_qtables = hd.n_qtables;
    d->total_blocks = pfv_total_blocks(w, h);
    if (!d->retframe.resize(pfv_frame_bytes(w, h))) {
        pfv_decoder_destroy(d);
        return fail(ctx, PFV_ERR_NOMEM, "pfv_decoder_create: pinned staging");
    }
    memset(d->retframe.data(), 0, (size_t)w * h);                              // VideoFrame::new (frame.rs:12-26): Y 0, U/V 128
    memset(d->retframe.data() + (size_t)w * h, 128, d->retframe.size() - (size_t)w * h);
    // the run streams of big packets are read on the device; the window stream and sets: with the first packet that takes the device form (dec_window_enqueue)
    d->entd.on = entd_take_options(ctx, &d->entd.force, &d->entd.sub_bits, &d->entd.launches, &d->entd.inner) && d->total_blocks > 0;
    const unsigned hw = std::thread::hardware_concurrency();
    if ((rc = pfv_decoder_set_lookahead(d, hw > 1 ? (int)std::min(4u, hw - 1) : 0))) {
        pfv_decoder_destroy(d);
        return rc;
    }
    *out = d;
    return PFV_OK;
}
}  // extern "C"

// ---- look-ahead machinery of pfv_decoder
static void dec_parse(pfv_decoder *d, DecEvent *e)   // any thread; touches only the event and the immutable stream
{
    const size_t tb = (size_t)d->total_blocks, cap = tb * 256 / 4;   // denser than 1 in 4: not worth a list
    e->dense = false;
    e->n_sparse = 0;
    e->dev_form = e->host_parse = false;
    auto parse_dense = [&]() -> int {
        if (!e->coef.resize(tb * 256)) return PFV_ERR_NOMEM;
        memset(e->coef.data(), 0, tb * 512);
        DenseSink sink{e->coef.data()};
        return parse_frame_to(e->type, e->payload, e->plen, d->total_blocks, d->n_qtables, e->mv.data(), e->has.data(), sink, e->qidx);
    };
    if (d->entd.on && (d->entd.force || e->plen >= kDecEntdMinBytes)) {   // the device reads the run streams: only the headers here
        if (!e->bytes.resize((size_t)e->plen + 32) || !e->pk.resize(1) || (e->type == 2 && (!e->mv.resize(tb * 2) || !e->has.resize(tb)))) {
            e->rc = PFV_ERR_NOMEM;
            return;
        }
        EdPacket &k = *e->pk.data();
        k.byte_off = 0; k.frame_off = 0;
        const EntdPrep r = entd_prepare(e->payload, e->plen, e->type, tb, d->n_qtables, d->entd.sub_bits, k, e->bytes.data());
        e->rc = r.rc;
        memcpy(e->qidx, r.qidx, 3);
        e->dev_form = true;
        e->host_parse = r.host_parse;
        if (!e->rc && e->host_parse) {   // the host parser decides about this one, here, on this thread
            e->dev_form = false;
            e->dense = true;
            e->rc = parse_dense();
        }
        return;
    }
    if (!e->idx.resize(cap) || !e->val.resize(cap) || (e->type == 2 && (!e->mv.resize(tb * 2) || !e->has.resize(tb)))) {
        e->rc = PFV_ERR_NOMEM;
        return;
    }
    SparseSink sink{e->idx.data(), e->val.data(), cap};
    e->rc = parse_frame_to(e->type, e->payload, e->plen, d->total_blocks, d->n_qtables, e->mv.data(), e->has.data(), sink, e->qidx);
    e->n_sparse = sink.n;
    if (e->rc != kSinkFull) return;
    e->dense = true;
    e->rc = parse_dense();
}
static void dec_worker(pfv_decoder *d)
{
    (void)hipSetDevice(d->ctx->device);   // the pinned landing zones are allocated from this thread
    std::unique_lock<std::mutex> lk(d->m);
    for (;;) {
        DecEvent *job = nullptr;
        for (size_t k = 0; k < d->count && !job; k++) {
            DecEvent *e = d->ring[(d->head + k) % d->ring.size()].get();
            if (e->state == DecEvent::QUEUED) job = e;
        }
        if (d->quit) return;
        if (!job) { d->cv_work.wait(lk); continue; }
        job->state = DecEvent::RUNNING;
        lk.unlock();
        dec_parse(d, job);
        lk.lock();
        job->state = DecEvent::DONE;
        d->cv_done.notify_all();
    }
}
// Walks packet headers from scan_pos exactly as the reference's loop would (dec.rs:174-222) and queues what it finds
// until the ring is full or an END / ERROR event is pending.  Caller holds the lock.
static void dec_scan(pfv_decoder *d)
{
    bool queued = false;
    while (d->count < d->ring.size() && !d->scan_stop) {
        DecEvent *e = d->ring[(d->head + d->count) % d->ring.size()].get();
        auto emit = [&](DecEvent::Kind kind, DecEvent::State st, size_t pos_after) {
            e->kind = kind; e->state = st; e->pos_after = pos_after;
            d->count++;
        };
        PfvPacket pk;
        const int rc = next_packet(d->data, d->len, d->scan_pos, pk);
        if (rc || pk.type == 0) {   // the stream ends here, as it should (EOF marker, :183-187) or not
            e->rc = rc; e->msg = pk.msg;
            emit(rc ? DecEvent::ERROR : DecEvent::END, DecEvent::DONE, pk.pos_after);
            d->scan_stop = true;
            break;
        }
        d->scan_pos = pk.pos_after;
        if (pk.type != 1 && pk.type != 2) continue;   // unknown packet: skipped (:216-219)
        if (pk.type == 1 && pk.plen == 0) {           // drop frame: nothing decoded, no callback (:190)
            emit(DecEvent::DROP, DecEvent::DONE, pk.pos_after);
            continue;
        }
        e->type = pk.type; e->payload = pk.payload; e->plen = pk.plen; e->rc = 0;
        emit(DecEvent::FRAME, DecEvent::QUEUED, pk.pos_after);
        queued = true;
    }
    if (queued) d->cv_work.notify_all();
}
// Forget everything scanned ahead and continue from `pos`.  Caller holds the lock.
static void dec_rewind(pfv_decoder *d, std::unique_lock<std::mutex> &lk, size_t pos)
{
    for (;;) {   // a parse in flight keeps pointers into its event: let it finish
        bool running = false;
        for (auto &e : d->ring) running |= e->state == DecEvent::RUNNING;
        if (!running) break;
        d->cv_done.wait(lk);
    }
    if (d->win_stream) (void)hipStreamSynchronize(d->win_stream);          // a window enqueued ahead reads its event's buffers
    for (DecWindow &w : d->win) w.owner = nullptr;
    for (auto &e : d->ring) e->state = DecEvent::FREE;
    d->head = d->count = 0;
    d->scan_pos = d->pos = pos;
    d->scan_stop = false;
}
static void dec_stop_workers(pfv_decoder *d)
{
    {
        std::lock_guard<std::mutex> lk(d->m);
        d->quit = true;
    }
    d->cv_work.notify_all();
    for (auto &t : d->workers) t.join();
    d->workers.clear();
    d->quit = false;
}

// where pfv_decoder_set_output_rgb's picture lands: pinned host memory, or device memory while the device output is on (either switch may come first)
static int dec_rgb_buffers(pfv_decoder *d)
{
    pfv_ctx *ctx = d->ctx;
    // the picture has the size of the frame it is made from: the resized one while pfv_decoder_set_output_size is on -- and is then made in
    // device memory on either output path (k_present_rgb from the packed resized frame)
    const size_t bytes = (d->scaler ? (size_t)d->out_w * d->out_h : (size_t)d->width * d->height) * 4;   // holds any format
    const bool dev_pic = d->rgb_on && (d->frame_dev || d->scaler);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (d->rgb_on && !d->frame_dev && !d->rgbframe.resize(bytes)) return fail(ctx, PFV_ERR_NOMEM, "pfv_decoder_set_output_rgb: pinned staging");
    if (d->rgb_dev && (!dev_pic || d->rgb_dev_cap < bytes)) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(d->rgb_dev); d->rgb_dev = nullptr; d->rgb_dev_cap = 0; }
    if (dev_pic && !d->rgb_dev) {
        HIP_TRY(ctx, hipMalloc((void **)&d->rgb_dev, bytes));
        d->rgb_dev_cap = bytes;
    }
    return PFV_OK;
}

extern "C" {

// Packets parsed ahead of the one being decoded, on `n_threads` worker threads (0: parse inline, no threads).  The
// default is min(4, hardware threads - 1).  Frames, order and error codes are those of the sequential loop.
PFV_API int pfv_decoder_set_lookahead(pfv_decoder *d, int n_threads)
{
    if (!d || n_threads < 0 || n_threads > 64) return fail(d ? d->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_decoder_set_lookahead: bad argument");
    dec_stop_workers(d);
    std::unique_lock<std::mutex> lk(d->m);
    dec_rewind(d, lk, d->pos);
    d->ring.clear();
    for (int i = 0; i < std::max(n_threads + 1, kDecWindows); i++) d->ring.emplace_back(new DecEvent());     // kDecWindows at least: the packets behind the current one are scanned (and, without threads, prepared by the caller's thread)
    lk.unlock();
    for (int i = 0; i < n_threads; i++) d->workers.emplace_back(dec_worker, d);
    return PFV_OK;
}

PFV_API void pfv_decoder_destroy(pfv_decoder *d)
{
    if (!d) return;
    dec_stop_workers(d);
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    if (d->win_stream) { (void)hipStreamSynchronize(d->win_stream); (void)hipStreamDestroy(d->win_stream); }
    if (d->frame_dev) (void)hipFree(d->frame_dev);
    if (d->rgb_dev) (void)hipFree(d->rgb_dev);
    if (d->scaled_dev) (void)hipFree(d->scaled_dev);
    pfv_scaler_destroy(d->scaler);
    for (DecWindow &w : d->win) w.destroy();
    pfv_dec_session_destroy(d->hot);
    delete d;
}
// on != 0: the decoded frame stays in device memory and the callback's y / u / v are DEVICE pointers to the packed frame (valid until the
// next advance call) -- for consumers on the GPU; the frame's download, more than half of a 4K call, is not paid
PFV_API int pfv_decoder_set_output_device(pfv_decoder *d, int on)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    pfv_ctx *ctx = d->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (on && !d->frame_dev) HIP_TRY(ctx, hipMalloc((void **)&d->frame_dev, pfv_frame_bytes(d->width, d->height)));
    if (!on && d->frame_dev) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(d->frame_dev); d->frame_dev = nullptr; }
    return dec_rgb_buffers(d);
}
// on != 0: the callback's y points to ONE tight picture in `format` (PFV_PIX_*, pfv_rgb_row_bytes x height bytes) and u, v are NULL -- in host
// memory, or in device memory under pfv_decoder_set_output_device(1); lifetime as the planar frame's.  Results, order and errors are unchanged.
PFV_API int pfv_decoder_set_output_rgb(pfv_decoder *d, int on, int format)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    if (on && !pfv_rgb_row_bytes(d->width, format)) return fail(d->ctx, PFV_ERR_BAD_ARG, "pfv_decoder_set_output_rgb: format must be PFV_PIX_RGB8, _RGBA8 or _BGRA8");
    d->rgb_on = on != 0;
    if (on) d->rgb_format = format;
    return dec_rgb_buffers(d);
}
// out-of-loop deblocking of the frames the callback receives: the session's switch (both output paths fetch the frame from the session)
PFV_API int pfv_decoder_set_deblock(pfv_decoder *d, int mode, const uint8_t strength[3])
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    const int rc = pfv_dec_set_deblock(d->hot, mode, strength);
    if (rc || mode == PFV_DEBLOCK_OFF || !d->scaler) return rc;
    return dec_present_scratch(d->hot, "pfv_decoder_set_deblock");   // the filtered picture waits there for k_scale: made here, never by an advance call
}
// w != 0: the callback's y, u, v point to the planes of ONE packed w x h frame, the decoded frame resized (kind: PFV_SCALE_*), and its width and
// height arguments are w and h; with pfv_decoder_set_output_rgb on, y is the picture of that resized frame.  In host memory, or in device memory
// under pfv_decoder_set_output_device(1).  w == 0 switches it off.  All scratch is made here.
PFV_API int pfv_decoder_set_output_size(pfv_decoder *d, int w, int h, int kind)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    pfv_ctx *ctx = d->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    pfv_scaler *sc = nullptr;
    int rc = PFV_OK;
    if (w != 0 && !(sc = pfv_scaler_create(ctx, d->width, d->height, w, h, kind, &rc))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // nothing reads the old tables or frame any more
    pfv_scaler_destroy(d->scaler);
    if (d->scaled_dev) { (void)hipFree(d->scaled_dev); d->scaled_dev = nullptr; }
    d->scaler = sc;
    d->out_w = sc ? w : 0; d->out_h = sc ? h : 0;
    if (sc) {
        HIP_TRY(ctx, hipMalloc((void **)&d->scaled_dev, pfv_frame_bytes(w, h)));
        if (!d->scaledframe.resize(pfv_frame_bytes(w, h))) return fail(ctx, PFV_ERR_NOMEM, "pfv_decoder_set_output_size: pinned staging");
        if (d->hot->db_mode && (rc = dec_present_scratch(d->hot, "pfv_decoder_set_output_size"))) return rc;
    }
    return dec_rgb_buffers(d);
}
PFV_API void pfv_decoder_entropy_counts(const pfv_decoder *d, long counts_out[2])
{
    if (!d || !counts_out) return;
    counts_out[0] = d->entd.packets_dev;
    counts_out[1] = d->entd.packets_host;
}
PFV_API int pfv_decoder_width(const pfv_decoder *d) { return d ? d->width : 0; }          // dec.rs:136-138
PFV_API int pfv_decoder_height(const pfv_decoder *d) { return d ? d->height : 0; }        // dec.rs:140-142
PFV_API int pfv_decoder_framerate(const pfv_decoder *d) { return d ? d->framerate : 0; }  // dec.rs:144-146
// Decoder::reset (src/dec.rs:148-152)
PFV_API int pfv_decoder_reset(pfv_decoder *d)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    std::unique_lock<std::mutex> lk(d->m);
    d->eof = false;
    dec_rewind(d, lk, d->reset_pos);
    return PFV_OK;
}

}  // extern "C"

// The window of packet e on set w: uploads, cleared coefficient array, k_entd_*, status download -- all on the window stream.
static int dec_window_enqueue(pfv_decoder *d, DecEvent *e, DecWindow &w)
{
    const int mrc = entd_windows_make(d->ctx, d->entd, d->win, &d->win_stream, 1, (size_t)d->total_blocks);
    if (mrc) return mrc;
    const size_t plen = e->plen;
    return entd_window_enqueue(d->ctx, d->entd, w, d->win_stream, e->pk.data(), e->bytes.data(), plen + 16, &plen, e->groups, e);
}
// One packet through the device's entropy stage, then the decode launch; before the frame is fetched, the window of the
// packet behind it -- if its headers are ready -- is put on the window stream, where it runs under this frame's decode and download.
static int dec_consume_entd(pfv_decoder *d, DecEvent *e)
{
    pfv_ctx *ctx = d->ctx;
    pfv_dec_session *hot = d->hot;
    DecEntd &v = d->entd;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    DecWindow *w = nullptr;
    for (DecWindow &x : d->win)
        if (x.owner == e) w = &x;
    if (!w) {                     // not enqueued ahead: now (every window is free or holds a packet behind this one; the last call ended with the stream idle)
        for (DecWindow &x : d->win)
            if (!w && !x.owner) w = &x;
        if (!w) { w = &d->win[0]; w->owner = nullptr; }
        if ((rc = dec_window_enqueue(d, e, *w))) { w->owner = nullptr; return rc; }
    }
    HIP_TRY(ctx, hipEventSynchronize(w->done));
    w->owner = nullptr;           // consumed (event objects are reused by the ring: a stale match would take this window for a later packet's)
    if (*w->status_host.data()) {   // the device stage is not certain about this payload: the host parser reads it and decides
        v.packets_host++;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // the staging list's last upload
        if ((rc = entd_host_parse(ctx, d->hp, *w, 0, e->payload, e->plen, e->type, d->n_qtables, e->mv.data(), e->has.data(), e->qidx, ctx->stream))) return rc;
    } else {
        v.packets_dev++;
    }
    rc = dec_step(hot, e->type == 2, w->mv_dev, w->has_dev, w->lists.coefs(), e->qidx);
    if (rc) return rc;
    // The packets behind this one: their windows (payload upload, k_hdr_*, k_entd_*, status) go onto the window stream now, where they run
    // under this frame's decode and download -- up to kDecWindows - 1 of them: one packet's window is a chain of a dozen small kernels
    // (~0.15 ms of latency for a 4K p-frame), so with a single window ahead the chain of packet t + 1 only started when packet t's decode was
    // launched and every frame waited for most of it.  The window just consumed is still being read by the decode launched above: it is not
    // among the free ones until this call has returned.
    for (size_t k = 1; k < (size_t)kDecWindows; k++) {
        std::unique_lock<std::mutex> lk(d->m);
        DecEvent *nx = d->count > k ? d->ring[(d->head + k) % d->ring.size()].get() : nullptr;
        if (!nx) break;
        if (nx->state == DecEvent::QUEUED && d->workers.empty()) {
            // no parser threads (pfv_decoder_set_lookahead(d, 0)): this thread reads the packet's first 19 bytes and stages its payload now,
            // while the decode just launched runs -- with the block headers read on the device that is all a big packet needs from the host
            nx->state = DecEvent::RUNNING;
            lk.unlock();
            dec_parse(d, nx);
            lk.lock();
            nx->state = DecEvent::DONE;
        }
        const bool ready = nx->state == DecEvent::DONE && nx->kind == DecEvent::FRAME && nx->dev_form && !nx->rc;
        const bool stop = nx->state != DecEvent::DONE || nx->kind == DecEvent::END || nx->kind == DecEvent::ERROR;
        lk.unlock();
        if (stop) break;
        if (!ready) continue;
        DecWindow *free_w = nullptr;
        bool has = false;
        for (DecWindow &x : d->win) {
            has = has || x.owner == nx;
            if (!free_w && !x.owner && &x != w) free_w = &x;
        }
        if (has) continue;
        if (!free_w) break;
        if (dec_window_enqueue(d, nx, *free_w) != PFV_OK) { free_w->owner = nullptr; break; }   // it will be tried again when its turn comes
    }
    return pfv_dec_check(hot);
}

extern "C" {
// Decoder::advance_frame (src/dec.rs:169-224).  Returns 1 = Ok(true), 0 = Ok(false) (EOF), negative = error.
// onvideo(user, y, u, v, width, height) is called for every decoded frame (not for drop frames).
PFV_API int pfv_decoder_advance_frame(pfv_decoder *d, pfv_video_cb onvideo, void *user)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    if (d->eof) return 0;
    std::unique_lock<std::mutex> lk(d->m);
    dec_scan(d);
    DecEvent *e = d->ring[d->head].get();
    while (e->state != DecEvent::DONE) {
        if (e->state == DecEvent::QUEUED) {   // nobody picked it up yet: parse it here
            e->state = DecEvent::RUNNING;
            lk.unlock();
            dec_parse(d, e);
            lk.lock();
            e->state = DecEvent::DONE;
        } else {
            d->cv_done.wait(lk);
        }
    }
    // consume the event; the slot stays reserved (FREE but not rescanned) until the device has read its buffers
    d->pos = e->pos_after;
    const DecEvent::Kind kind = e->kind;
    if (kind == DecEvent::END || kind == DecEvent::ERROR) {
        const int rc = e->rc;
        const char *msg = e->msg;
        dec_rewind(d, lk, d->pos);   // nothing was scanned past it; the next call rescans from pos like the reference
        if (kind == DecEvent::END) {
            d->eof = true;
            return 0;
        }
        return fail(d->ctx, rc, msg);
    }
    int rc = PFV_OK;
    if (kind == DecEvent::FRAME) {
        lk.unlock();   // workers keep parsing the packets behind this one while the device decodes it
        rc = e->rc;
        if (rc) rc = fail(d->ctx, rc, rc == PFV_ERR_NOMEM ? "pinned staging for a parsed packet" : "malformed packet payload");
        if (!rc && e->host_parse && !e->dev_form) d->entd.packets_host++;   // a packet of device size the host parser had to read (degenerate table, 64 MiB and more)
        if (!rc && e->dev_form) {
            rc = dec_consume_entd(d, e);
            if (rc && !d->entd.ready && !d->entd.force) {
                // PFV_ENTROPY_DECODE_AUTO and the window stream / sets could not be made (they are created with the first packet that takes the
                // device form): the device stage is switched off for this decoder and the host parser reads this packet -- and the ones the
                // parser threads have already prepared in device form, each when its turn comes.  An error only under PFV_ENTROPY_DECODE_DEVICE.
                (void)hipGetLastError();
                d->entd.on = false;
                dec_parse(d, e);
                rc = e->rc;
                if (rc) rc = fail(d->ctx, rc, rc == PFV_ERR_NOMEM ? "pinned staging for a parsed packet" : "malformed packet payload");
                else d->entd.packets_host++;
            }
        }
        if (rc || e->dev_form)
            ;
        else if (e->dense)
            rc = e->type == 1 ? pfv_dec_iframe(d->hot, e->coef.data(), e->qidx)
                              : pfv_dec_pframe(d->hot, e->mv.data(), e->has.data(), e->coef.data(), e->qidx);
        else
            rc = e->type == 1 ? pfv_dec_iframe_sparse(d->hot, e->idx.data(), e->val.data(), e->n_sparse, e->qidx)
                              : pfv_dec_pframe_sparse(d->hot, e->mv.data(), e->has.data(), e->idx.data(), e->val.data(),
                                                      e->n_sparse, e->qidx);
        if (!rc && d->scaler) {      // pfv_decoder_set_output_size: one k_scale from what pfv_dec_get_frame_dev would return, then the picture of that frame if asked for
            const size_t fb = pfv_frame_bytes(d->out_w, d->out_h), pic = pfv_rgb_row_bytes(d->out_w, d->rgb_format) * (size_t)d->out_h;
            rc = dec_scaled_win(d->hot, d->scaler, 0, 1, nullptr, 0, d->scaled_dev, fb);
            if (!rc && d->rgb_on) rc = pfv_frames_to_rgb_dev(d->ctx, d->out_w, d->out_h, 1, d->scaled_dev, PFV_FRAME_PACKED, 0, d->rgb_dev, d->rgb_format, 0, 0);
            if (!rc && !d->frame_dev) {
                const hipError_t he = d->rgb_on ? hipMemcpyAsync(d->rgbframe.data(), d->rgb_dev, pic, hipMemcpyDeviceToHost, d->ctx->stream)
                                                : hipMemcpyAsync(d->scaledframe.data(), d->scaled_dev, fb, hipMemcpyDeviceToHost, d->ctx->stream);
                if (he != hipSuccess) rc = hip_fail(d->ctx, he, "download of the resized frame");
            }
            if (!rc) rc = pfv_ctx_sync(d->ctx);
        } else if (!rc && d->rgb_on) {      // pfv_decoder_set_output_rgb: one picture instead of the planes, on either side
            if (d->frame_dev) {
                rc = pfv_dec_get_frame_rgb_dev(d->hot, d->rgb_dev, d->rgb_format, 0, 0);
                if (!rc) rc = pfv_ctx_sync(d->ctx);
            } else {
                rc = pfv_dec_get_frame_rgb(d->hot, d->rgbframe.data(), d->rgb_format);
            }
        } else if (!rc && d->frame_dev) {   // pfv_decoder_set_output_device: the retframe stays in device memory
            rc = pfv_dec_get_frame_dev(d->hot, d->frame_dev);
            if (!rc) rc = pfv_ctx_sync(d->ctx);
        } else if (!rc) {
            rc = pfv_dec_get_frame(d->hot, d->retframe.data());   // crop blits (:195-197, 209-211)
        }
        lk.lock();
    }
    e->state = DecEvent::FREE;
    d->head = (d->head + 1) % d->ring.size();
    d->count--;
    dec_scan(d);       // refill the freed slot right away
    lk.unlock();
    if (rc) return rc;
    if (kind == DecEvent::FRAME && onvideo && d->rgb_on) {
        onvideo(user, d->frame_dev ? d->rgb_dev : d->rgbframe.data(), nullptr, nullptr, d->scaler ? d->out_w : d->width, d->scaler ? d->out_h : d->height);
    } else if (kind == DecEvent::FRAME && onvideo && d->scaler) {
        const size_t ny = (size_t)d->out_w * d->out_h, nc = (size_t)(d->out_w / 2) * (d->out_h / 2);
        const uint8_t *f = d->frame_dev ? d->scaled_dev : d->scaledframe.data();
        onvideo(user, f, f + ny, f + ny + nc, d->out_w, d->out_h);
    } else if (kind == DecEvent::FRAME && onvideo) {
        size_t ny = (size_t)d->width * d->height, nc = (size_t)(d->width / 2) * (d->height / 2);
        const uint8_t *f = d->frame_dev ? d->frame_dev : d->retframe.data();
        onvideo(user, f, f + ny, f + ny + nc, d->width, d->height);
    }
    return 1;
}

// Decoder::advance_delta (src/dec.rs:154-167)
PFV_API int pfv_decoder_advance_delta(pfv_decoder *d, double delta, pfv_video_cb onvideo, void *user)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    d->delta_accum += delta;
    double delta_per_frame = 1.0 / (double)d->framerate;
    while (d->delta_accum >= delta_per_frame) {
        int rc = pfv_decoder_advance_frame(d, onvideo, user);
        if (rc <= 0) return rc;
        d->delta_accum -= delta_per_frame;
    }
    return 1;
}

}  // extern "C"
