// pfv_gop.hip -- GOP-batched stream objects: what both use and pfv_gop_encoder; pfv_gop_decoder is in pfv_gop_decoder.hip (included by
// pfv_capi.hip; uses its sessions, PinnedBuf and the host parsers).
//
// enc::Encoder / dec::Decoder (src/enc.rs:12-188, src/dec.rs:15-224) for ONE stream, with the independent GOPs of the stream as the
// slots of every launch.  encode_iframe never reads prev_frame and overwrites all three planes of it (src/enc.rs:84-97);
// decode_plane_into overwrites the whole framebuffer (src/common.rs:477-496): the runs I P P ... of a stream share nothing, so frame
// t of EVERY run of a batch goes through one launch per stage instead of one launch per frame.  A single 4K stream then fills the
// device like 20 streams do (bench.py --workload config5: 0.97 G -> 1.39 G macroblocks/s at kernel scope).  The bytes written and the
// frames delivered are those of the frame-by-frame objects (pfv_encoder / pfv_decoder); only WHEN they appear differs: a packet
// leaves when its batch is complete.
//
//   batch        up to max_gops runs ("groups") of up to max_gop_frames frames; a group starts at an i-frame.  A run longer than
//                max_gop_frames continues in slot 0 of the next batch (its reference frame is carried over, one device copy), and so
//                does a stream that starts with p-frames (prev_frame = new_padded, src/enc.rs:46).
//   frame step   t = 0 .. longest group - 1: the slots whose group has a frame t, as maximal runs of neighbouring slots of one frame
//                type (normally ONE launch: all groups are equally long but the last).  The ping-pong index of the session
//                flips once per step; a slot that sits a step out never reads its stale side (its next frame is an i-frame, or the
//                state is copied explicitly: failed packets on the decoder side).
#pragma once

// wall-clock accounting of where a GOP-batched object spends its host time (pfv_gop_*_stats): cheap (two clock reads per section)
struct GopClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap()
    {
        const auto t1 = std::chrono::steady_clock::now();
        const double s = std::chrono::duration<double>(t1 - t0).count();
        t0 = t1;
        return s;
    }
};

// PFV_GOP_TRACE=1: a host-side log of the encoder's steps (seconds since the object was created) on stderr -- where a rocprofv3 trace would
// distort the host's own timing
struct GopTrace {
    bool on = getenv("PFV_GOP_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what, long a = 0, long b = 0) const
    {
        if (on) fprintf(stderr, "[pfv gop %9.3f ms] %s %ld %ld\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3, what, a, b);
    }
};

struct GopPacket {
    uint8_t type;     // 1 i-frame, 2 p-frame, 3 drop frame (src/enc.rs:175-180)
    int slot, t;
};

struct GopEncBatch {
    std::vector<int> len;              // frames per group; slot = index
    std::vector<uint8_t> first_type;   // 1: the group starts with an i-frame; 2: it continues a run (or the stream starts with p-frames)
    std::vector<GopPacket> order;      // packets of the batch in stream order
    bool in_flight = false;            // kernels enqueued, payloads not yet collected
    int steps = 0;                     // frame steps enqueued (longest group)
    uint8_t *frames_dev = nullptr;     // [max_gop_frames][max_gops][frame_bytes]
    // where each frame of the batch lies: its place in frames_dev, or -- device frames taken BY REFERENCE -- the caller's own buffer
    PinnedBuf<const uint8_t *> slots_host;      // [max_gop_frames][max_gops]
    const uint8_t **slots_dev = nullptr;
    bool by_ref = false;               // some frame of the batch is read where the caller left it
    uint8_t *arena = nullptr;          // retained payloads of the batch
    size_t arena_cap = 0;              // its size: grows (this batch's arena alone) after a batch outgrew it
    uint8_t *cont_save = nullptr;      // the reference frame slot 0 continued from, saved at submit (one padded frame; allocated with the first such batch):
    bool cont_saved = false;           //   what a batch that outgrew its arena is encoded again from (gop_enc_redo)
    std::vector<uint8_t> redo;         // the packets' payloads of such a batch, made again frame by frame; the pending segments point into it
    EntEntry *entries_dev = nullptr;   // [max_gop_frames][max_gops]
    unsigned long long *cursor_dev = nullptr;
    hipEvent_t ev_uploaded = nullptr, ev_done = nullptr, ev_dev_frames = nullptr;
    bool dev_frames = false;           // frames were copied on the caller's stream: the batch's kernels wait for ev_dev_frames
    // the payloads come over step by step, under the kernels of the steps behind them: after step t the arena's fill level is copied to
    // cursor_steps[t] (page-locked) and ev_step[t] recorded; whoever next looks at the batch (any encode call, the collection) fetches the
    // bytes the finished steps added (gop_enc_fetch)
    std::vector<hipEvent_t> ev_step;
    PinnedBuf<unsigned long long> cursor_steps;
    int steps_fetched = 0;
    size_t fetched_bytes = 0;
    PinnedBuf<uint8_t> payload_host;   // the batch's payloads on the host (page-locked): the pending segments point into it
    std::vector<uint8_t> heads;        // 5 bytes per packet of the batch
    void clear() { len.clear(); first_type.clear(); order.clear(); in_flight = false; dev_frames = false; by_ref = false; steps = 0; steps_fetched = 0; fetched_bytes = 0; }
    int frames() const { int n = 0; for (int l : len) n += l; return n; }
};

struct pfv_gop_encoder {
    // ctx: the encoder's OWN launch context (a stream of its own for the batches' kernels); user: the context the caller created the encoder
    // on -- frames that lie in device memory are copied on ITS stream (the *_dev ordering), so the copies of the batch being filled run under
    // the kernels of the batch in flight instead of queueing behind them
    pfv_ctx *ctx = nullptr;      // ctx->owner = the caller's context, or nullptr once that has been destroyed
    pfv_enc_session *hot = nullptr;
    int width = 0, height = 0, max_gops = 0, max_len = 0;
    size_t frame_bytes = 0, total_blocks = 0, arena_cap = 0;       // arena_cap: what a batch's arena starts with
    bool explicit_budget = false;          // the caller gave pfv_gop_encoder_create a payload budget: outgrowing it is an error, not a reason to grow
    int quality = 0;
    long batches_redone = 0;
    std::vector<uint32_t> redo_sizes;      // payload bytes of the packets of the batch made again, in stream order (drop frames left out)
    GopEncBatch batch[2];
    int cur = 0;                           // batch being filled
    hipStream_t copy_stream = nullptr;     // plane uploads
    hipStream_t down_stream = nullptr;     // payload downloads (its own stream: an upload's wait must not queue behind them)
    int16_t *coef = nullptr;               // encode outputs of one step, max_gops wide
    int8_t *mv = nullptr;
    uint8_t *has = nullptr;
    bool cont_valid = false;               // a group is open across the batch boundary: where its prev_frame lives
    int cont_buf = 0, cont_slot = 0;
    PinnedBuf<EntEntry> entries_host;
    unsigned long long *cursor_host = nullptr;   // page-locked
    // the writer side: bytes produced and not yet handed over = `out` (contiguous) followed by `segs` (packet headers and payloads where
    // they lie: a batch's payloads stay in its page-locked landing zone until the batch slot is collected again)
    std::vector<uint8_t> out, drained;
    std::vector<pfv_iovec> segs, segs_drained;
    unsigned segs_in = 0;                  // bit b: pending segments point into batch[b]'s landing zone / header bytes
    bool finished = false, failed = false;
    bool frames_by_ref = false;            // pfv_gop_encoder_set_frames_by_reference
    long frames_in = 0, batches = 0, frames_by_reference = 0;
    // seconds: [0] waiting for plane uploads, [1] enqueueing batches, [2] waiting for a batch's kernels, [3] payloads device -> host,
    // [4] packet assembly
    double stats[5] = {0, 0, 0, 0, 0};
    GopTrace trace;
};

// ---- helpers of both objects
template <class F>
static void gop_runs(const std::vector<int> &key, F &&fn)   // maximal runs of equal non-negative keys over neighbouring slots
{
    const int n = (int)key.size();
    for (int a = 0; a < n;) {
        if (key[(size_t)a] < 0) { a++; continue; }
        int b = a + 1;
        while (b < n && key[(size_t)b] == key[(size_t)a]) b++;
        fn(a, b - a, key[(size_t)a]);
        a = b;
    }
}

// the options of the caller's context as they stand now (the launches read them from the encoder's own)
static void gop_enc_take_options(pfv_gop_encoder *e)
{
    pfv_ctx *k = e->ctx;
    const pfv_ctx *u = e->ctx->owner;
    if (!u) return;          // the caller's context is gone: the options stay as they were last taken
    k->opt_enc_transform = u->opt_enc_transform;
    k->opt_tile_compaction = u->opt_tile_compaction;
    k->opt_lane_mapping = u->opt_lane_mapping;
}

// every frame step of a batch, enqueued without a host round trip
static int gop_enc_submit(pfv_gop_encoder *e, GopEncBatch &B)
{
    pfv_ctx *ctx = e->ctx;
    pfv_enc_session *s = e->hot;
    const int G = (int)B.len.size();
    if (G == 0 || B.in_flight) return PFV_OK;
    GopClock clk;
    e->trace("submit begin: batch, groups", (long)(&B - e->batch), G);
    gop_enc_take_options(e);
    HIP_TRY(ctx, hipEventRecord(B.ev_uploaded, e->copy_stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, B.ev_uploaded, 0));
    if (B.dev_frames) {
        if (!ctx->owner) return fail(ctx, PFV_ERR_STATE, "the context the encoder was created on has been destroyed: its device-frame copies have no stream");
        HIP_TRY(ctx, hipEventRecord(B.ev_dev_frames, ctx->owner->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, B.ev_dev_frames, 0));
    }
    const size_t pad = (size_t)s->geom.pad_frame_bytes;
    B.cont_saved = false;
    if (B.first_type[0] == 2 && e->cont_valid) {   // slot 0 continues the run the previous batch left open: carry its reference frame over
        const uint8_t *src = s->prev[e->cont_buf] + (size_t)e->cont_slot * pad;
        uint8_t *dst = s->prev[s->cur];
        if (src != dst) HIP_TRY(ctx, hipMemcpyAsync(dst, src, pad, hipMemcpyDeviceToDevice, ctx->stream));
        if (!e->explicit_budget) {                 // and keep a copy: what the batch is encoded again from should it outgrow its arena
            if (!B.cont_save) HIP_TRY(ctx, hipMalloc((void **)&B.cont_save, pad));
            HIP_TRY(ctx, hipMemcpyAsync(B.cont_save, src, pad, hipMemcpyDeviceToDevice, ctx->stream));
            B.cont_saved = true;
        }
    }
    HIP_TRY(ctx, hipMemsetAsync(B.cursor_dev, 0, sizeof(unsigned long long), ctx->stream));
    if (B.by_ref)    // the batch's table of frame pointers (page-locked -> device, ahead of the kernels on their stream)
        HIP_TRY(ctx, hipMemcpyAsync(B.slots_dev, B.slots_host.data(), (size_t)e->max_len * (size_t)e->max_gops * sizeof(const uint8_t *), hipMemcpyHostToDevice, ctx->stream));
    int steps = 0;
    for (int l : B.len) steps = std::max(steps, l);
    const int cur0 = s->cur;
    std::vector<int> key((size_t)G);
    EntFrame f{};
    f.cap_bytes = s->ent_cap;
    for (int t = 0; t < steps; t++) {
        for (int k = 0; k < G; k++) key[(size_t)k] = B.len[(size_t)k] > t ? (t == 0 ? B.first_type[(size_t)k] : 2) : -1;
        const uint8_t *frames_t = B.frames_dev + (size_t)t * (size_t)e->max_gops * e->frame_bytes;
        int rc = PFV_OK;
        gop_runs(key, [&](int first, int count, int type) {
            if (!rc) rc = enc_launch(s, type == 2, first, count, frames_t, e->mv, e->has, e->coef, B.by_ref ? B.slots_dev + (size_t)t * (size_t)e->max_gops : nullptr);
            if (!rc) rc = ent_pack_win(s, type == 2, first, count, e->mv, e->has, e->coef);
            if (rc) return;
            EntEntry *ent = B.entries_dev + (size_t)t * (size_t)e->max_gops + (size_t)first;
            EntBufs b = s->ent;
            b.sizes += first;
            b.payload += (size_t)first * (size_t)s->ent_cap;
            hipLaunchKernelGGL(k_ent_retain, dim3(1), dim3(64), 0, ctx->stream, b.sizes, count, B.cursor_dev, (unsigned long long)B.arena_cap, ent, B.cursor_steps.data() + t);
            f.n_streams = count;
            hipLaunchKernelGGL(k_ent_gather_entries, dim3(32, (unsigned)count), dim3(kEntThreads), 0, ctx->stream, f, b, ent, B.arena);
            rc = launch_check(ctx, "k_ent_retain / k_ent_gather_entries");
        });
        if (rc) return rc;
        s->cur ^= 1;
        HIP_TRY(ctx, hipEventRecord(B.ev_step[(size_t)t], ctx->stream));
    }
    // the last group may go on in the next batch: its reference frame is in the buffer its last step wrote
    e->cont_valid = true;
    e->cont_slot = G - 1;
    e->cont_buf = (cur0 + B.len[(size_t)G - 1]) & 1;
    HIP_TRY(ctx, hipEventRecord(B.ev_done, ctx->stream));
    B.steps = steps;
    B.steps_fetched = 0;
    B.fetched_bytes = 0;
    B.in_flight = true;
    e->batches++;
    e->stats[1] += clk.lap();
    e->trace("submit end: batch, steps", (long)(&B - e->batch), steps);
    return PFV_OK;
}

// pending segments -> the contiguous byte vector (callers that did not take them before their buffers are needed again, and the
// contiguous drain / bytes calls)
static void gop_enc_materialize(pfv_gop_encoder *e)
{
    size_t n = 0;
    for (const pfv_iovec &v : e->segs) n += v.len;
    e->out.reserve(e->out.size() + n);
    for (const pfv_iovec &v : e->segs) e->out.insert(e->out.end(), v.data, v.data + v.len);
    e->segs.clear();
    e->segs_in = 0;
}

// The payload bytes the finished steps of an in-flight batch added to its arena: device -> the batch's landing zone, on the download stream.
// wait: every step (the batch is being collected); otherwise only the steps whose event has fired (called from the encode calls, so that
// the bytes travel under the kernels of the steps and the batch behind them instead of after the last kernel).
static int gop_enc_fetch(pfv_gop_encoder *e, GopEncBatch &B, bool wait)
{
    pfv_ctx *ctx = e->ctx;
    if (!B.in_flight) return PFV_OK;
    if (B.steps_fetched < B.steps && (e->segs_in & (1u << (unsigned)(&B - e->batch)))) gop_enc_materialize(e);   // segments of the batch's previous use that nobody took yet
    while (B.steps_fetched < B.steps) {
        hipEvent_t ev = B.ev_step[(size_t)B.steps_fetched];
        if (wait) HIP_TRY(ctx, hipEventSynchronize(ev));
        else if (hipEventQuery(ev) != hipSuccess) { (void)hipGetLastError(); break; }
        const size_t upto = std::min((size_t)B.cursor_steps.data()[B.steps_fetched], B.arena_cap);
        if (upto > B.payload_host.size()) {
            // the landing zone is too small (page-locking is slow: it grows in big steps): what has arrived moves to the new one
            HIP_TRY(ctx, hipStreamSynchronize(e->down_stream));
            PinnedBuf<uint8_t> bigger;
            if (!bigger.resize(std::min(B.arena_cap, upto + upto / 2 + ((size_t)4 << 20)))) return fail(ctx, PFV_ERR_NOMEM, "pinned payload staging");
            memcpy(bigger.data(), B.payload_host.data(), B.fetched_bytes);
            B.payload_host.swap(bigger);
        }
        if (upto > B.fetched_bytes) {
            HIP_TRY(ctx, hipMemcpyAsync(B.payload_host.data() + B.fetched_bytes, B.arena + B.fetched_bytes, upto - B.fetched_bytes, hipMemcpyDeviceToHost, e->down_stream));
        }
        if (e->trace.on) (void)hipLaunchHostFunc(e->down_stream, [](void *p) { (*(const GopTrace *)p)("   ... a download arrived (stream 1)"); }, &e->trace);
        e->trace(wait ? "download issued (waited): step, bytes" : "download issued (polled): step, bytes", B.steps_fetched, (long)(upto - std::min(upto, B.fetched_bytes)));
        B.fetched_bytes = std::max(B.fetched_bytes, upto);
        B.steps_fetched++;
    }
    return PFV_OK;
}

// A batch whose payloads outgrew its arena (default budget): every packet of it is made again, one frame at a time, on a one-stream session of
// its own -- the frames still lie where the batch read them (its frame array, or the caller's buffers under the by-reference contract), a
// group starts with an i-frame or, slot 0, from the reference frame saved at submit.  Same arithmetic, same bytes; serial and slow, which is
// fine for what is at most a once-per-content event: the batch's arena then grows so that the batches behind it fit.
static int gop_enc_redo(pfv_gop_encoder *e, GopEncBatch &B)
{
    pfv_ctx *ctx = e->ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the batch behind this one may be running: it shares coef / mv / has with the pass below
    HIP_TRY(ctx, hipStreamSynchronize(e->down_stream));
    pfv_enc_session *r = nullptr;
    int rc = pfv_enc_session_create(ctx, e->width, e->height, e->quality, 1, &r);
    if (!rc) rc = pfv_enc_entropy_enable(r, 0);
    if (!rc) rc = pfv_enc_session_set_motion_search(r, e->hot->search_mode, e->hot->search_radius);   // the batch's own search: same bytes
    B.redo.clear();
    e->redo_sizes.clear();
    const size_t pad = (size_t)e->hot->geom.pad_frame_bytes;
    int last_slot = -1;
    for (size_t i = 0; !rc && i < B.order.size(); i++) {
        const GopPacket &p = B.order[i];
        if (p.type == 3) continue;
        if (p.slot != last_slot && p.type == 2) {             // a group that starts with a p-frame: slot 0 continuing the run before the batch
            if (B.cont_saved) rc = hipMemcpyAsync((void *)pfv_enc_prev_frame_dev(r, 0), B.cont_save, pad, hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess ? PFV_OK : hip_fail(ctx, hipGetLastError(), "gop_enc_redo");
            // (no saved frame: the stream itself starts with p-frames, and a new session's prev_frame is the state they start from, src/frame.rs:38-43)
        }
        last_slot = p.slot;
        const uint8_t *f = B.slots_host.data()[(size_t)p.t * (size_t)e->max_gops + (size_t)p.slot];
        if (!rc) rc = p.type == 1 ? pfv_enc_iframe_dev(r, f, e->coef) : pfv_enc_pframe_dev(r, f, e->mv, e->has, e->coef);
        if (!rc) rc = p.type == 1 ? pfv_enc_pack_iframe_dev(r, e->coef) : pfv_enc_pack_pframe_dev(r, e->mv, e->has, e->coef);
        uint32_t size = 0;
        if (!rc) rc = pfv_enc_payload_sizes(r, &size);          // synchronises; PFV_ERR_FORMAT for a coefficient of more than 15 size bits
        if (rc) break;
        const size_t at = B.redo.size();
        B.redo.resize(at + size);
        if (size) rc = pfv_enc_payload_fetch(r, 0, B.redo.data() + at, size);
        e->redo_sizes.push_back(size);
    }
    pfv_enc_session_destroy(r);
    if (rc) return rc;
    e->batches_redone++;
    // this batch's arena for the batches to come: one and a half times what the batch needed (every payload on a 16-byte boundary)
    const size_t need = B.redo.size() + 16 * e->redo_sizes.size();
    const size_t want = ((need + need / 2) + 15) & ~(size_t)15;
    if (want > B.arena_cap) {
        uint8_t *bigger = nullptr;
        if (hipMalloc((void **)&bigger, want) == hipSuccess) {
            (void)hipFree(B.arena);
            B.arena = bigger;
            B.arena_cap = want;
        } else {
            (void)hipGetLastError();                            // it stays as it is; the next batch that outgrows it is made again like this one
        }
    }
    return PFV_OK;
}

// wait for a batch, bring its payloads over and write its packets in stream order
static int gop_enc_collect(pfv_gop_encoder *e, GopEncBatch &B)
{
    pfv_ctx *ctx = e->ctx;
    const unsigned slot_bit = 1u << (unsigned)(&B - e->batch);
    if (e->segs_in & slot_bit) gop_enc_materialize(e);   // this slot's landing zone is about to be overwritten: segments nobody took yet
    //                                                     are copied out first
    if (!B.in_flight) {   // nothing was encoded: only drop frames can be pending
        gop_enc_materialize(e);
        for (const GopPacket &p : B.order)
            if (p.type == 3) put_packet(e->out, 1, nullptr, 0);
        B.clear();
        return PFV_OK;
    }
    const size_t n_ent = (size_t)B.steps * (size_t)e->max_gops;
    // the batch is complete on the device; its results come over on the copy stream (idle: every upload was waited for), NOT behind
    // the kernels of the next batch, which may already be queued on the context's stream
    GopClock clk;
    {   // the steps' payloads as they complete (most have come over already, under the kernels), then the batch's entry table
        const int frc = gop_enc_fetch(e, B, true);
        if (frc) { e->failed = true; return frc; }
    }
    HIP_TRY(ctx, hipEventSynchronize(B.ev_done));
    e->stats[2] += clk.lap();
    e->trace("batch done on the device: batch", (long)(&B - e->batch));
    HIP_TRY(ctx, hipMemcpyAsync(e->entries_host.data(), B.entries_dev, n_ent * sizeof(EntEntry), hipMemcpyDeviceToHost, e->down_stream));
    HIP_TRY(ctx, hipStreamSynchronize(e->down_stream));
    int rc = PFV_OK;
    for (const GopPacket &p : B.order) {
        if (p.type == 3) continue;
        const uint32_t sz = e->entries_host.data()[(size_t)p.t * (size_t)e->max_gops + (size_t)p.slot].size;
        if (sz == kEntErrOversize) rc = PFV_ERR_FORMAT;
        else if (sz == kEntErrCapacity && rc == PFV_OK) rc = PFV_ERR_NOMEM;
    }
    if (rc == PFV_ERR_NOMEM && !e->explicit_budget) {
        // the batch outgrew its arena and nobody asked for a bound: Encoder::encode_pframe cannot fail for size (src/enc.rs:125-173), so the
        // batch's packets are made again, frame by frame, and this arena grows for the batches to come
        rc = gop_enc_redo(e, B);
        if (rc) { e->failed = true; return rc; }
        e->stats[3] += clk.lap();
        B.heads.resize(B.order.size() * 5);
        e->segs_in |= slot_bit;
        size_t hi = 0, k = 0, off = 0;
        for (const GopPacket &p : B.order) {      // packets in stream order: 5 header bytes, then the payload where gop_enc_redo left it
            uint8_t *h = &B.heads[hi];
            hi += 5;
            const uint32_t size = p.type == 3 ? 0u : e->redo_sizes[k++];   // type 3, a drop frame: an empty i-frame packet (src/enc.rs:175-180)
            put_packet_head(h, p.type == 3 ? 1 : p.type, size);
            e->segs.push_back(pfv_iovec{h, 5});
            if (size) e->segs.push_back(pfv_iovec{B.redo.data() + off, (size_t)size});
            off += size;
        }
        e->stats[4] += clk.lap();
        B.clear();
        return PFV_OK;
    }
    if (rc) {
        e->failed = true;
        return fail(ctx, rc, rc == PFV_ERR_FORMAT ? "coefficient needs more than 15 size bits (src/rle.rs:44)"
                                                  : "the batch's packet payloads exceed the payload budget given to pfv_gop_encoder_create");
    }
    e->stats[3] += clk.lap();
    e->trace("payloads on the host: batch, bytes", (long)(&B - e->batch), (long)B.fetched_bytes);
    // packets in stream order as segments: 5 header bytes (src/enc.rs:301-305, :453-457), then the payload where it lies
    B.heads.resize(B.order.size() * 5);
    e->segs_in |= slot_bit;
    size_t hi = 0;
    for (const GopPacket &p : B.order) {
        uint8_t *h = &B.heads[hi];
        hi += 5;
        if (p.type == 3) {                                                // drop frame: an empty i-frame packet (src/enc.rs:175-180)
            put_packet_head(h, 1, 0);
            e->segs.push_back(pfv_iovec{h, 5});
            continue;
        }
        const EntEntry &en = e->entries_host.data()[(size_t)p.t * (size_t)e->max_gops + (size_t)p.slot];
        put_packet_head(h, p.type, en.size);
        e->segs.push_back(pfv_iovec{h, 5});
        if (en.size) e->segs.push_back(pfv_iovec{B.payload_host.data() + en.offset, (size_t)en.size});
    }
    e->stats[4] += clk.lap();
    B.clear();
    return PFV_OK;
}

// the batch being filled is complete: enqueue it, turn to the other one (collecting what it still holds)
static int gop_enc_rotate(pfv_gop_encoder *e)
{
    int rc = gop_enc_submit(e, e->batch[e->cur]);
    if (rc) { e->failed = true; return rc; }
    e->cur ^= 1;
    return gop_enc_collect(e, e->batch[e->cur]);
}

static int gop_enc_frame_inner(pfv_gop_encoder *e, int type, const uint8_t *y, const uint8_t *u, const uint8_t *v, bool on_device);
static int gop_enc_frame(pfv_gop_encoder *e, int type, const uint8_t *y, const uint8_t *u, const uint8_t *v, bool on_device = false)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    pfv_ctx *ctx = e->ctx;
    if (!y || !u || !v) return fail(ctx, PFV_ERR_BAD_ARG, "null plane");
    if (e->finished) return fail(ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:80)");
    if (e->failed) return fail(ctx, PFV_ERR_STATE, "an earlier batch failed: the stream is incomplete");
    const int rc = gop_enc_frame_inner(e, type, y, u, v, on_device);
    if (rc) e->failed = true;          // a frame is missing from the stream from here on (the reference's Encoder would have panicked)
    return rc;
}
static int gop_enc_frame_inner(pfv_gop_encoder *e, int type, const uint8_t *y, const uint8_t *u, const uint8_t *v, bool on_device)
{
    pfv_ctx *ctx = e->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GopEncBatch *B = &e->batch[e->cur];
    int rc = PFV_OK;
    if (type == 1) {
        if ((int)B->len.size() == e->max_gops) { if ((rc = gop_enc_rotate(e))) return rc; B = &e->batch[e->cur]; }
        B->len.push_back(0); B->first_type.push_back(1);
    } else if (B->len.empty() || B->len.back() == e->max_len) {
        // a p-frame with no open group in this batch: the run continues from the previous batch (or the stream starts with p-frames)
        if (!B->len.empty()) { if ((rc = gop_enc_rotate(e))) return rc; B = &e->batch[e->cur]; }
        B->len.push_back(0); B->first_type.push_back(2);
    }
    if ((rc = gop_enc_fetch(e, e->batch[e->cur ^ 1], false))) return rc;      // the batch in flight: the payloads of its finished steps start travelling
    const int slot = (int)B->len.size() - 1, t = B->len.back()++;
    // the three planes go straight to their place in the step's frame array (VideoFrame, src/frame.rs:3-9: no packing on the host)
    uint8_t *dst = B->frames_dev + ((size_t)t * (size_t)e->max_gops + (size_t)slot) * e->frame_bytes;
    B->slots_host.data()[(size_t)t * (size_t)e->max_gops + (size_t)slot] = dst;
    const size_t ny = (size_t)e->width * e->height, nc = (size_t)(e->width / 2) * (e->height / 2);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;   // *_dev: a frame that is in device memory already
    if (on_device) {
        // ordered on the stream of the CALLER's context like every *_dev call of the library (behind whatever produced the frame there, ahead of
        // whatever overwrites it there), and without a host wait: the batch's kernels -- on the encoder's own stream -- wait for an event
        // recorded behind the batch's last copy.  (Round 4 copied on the upload stream and waited for it per frame: 300 waits were a third
        // of the 22 ms a 300-frame 4K clip took; until the encoder had a stream of its own the copies queued behind the previous batch's kernels.)
        if (!ctx->owner) return fail(ctx, PFV_ERR_STATE, "the context the encoder was created on has been destroyed (pfv_gop_encoder_encode_*_dev copies on its stream)");
        if (e->frames_by_ref && ((uintptr_t)y & 15) == 0) {
            // by reference: no copy at all -- the step's kernels read the frame where it lies (FrameGeom::src_slots).  The caller keeps it
            // valid and unchanged until the batch has been collected (pfv_hip_ext.h: pfv_gop_encoder_set_frames_by_reference)
            B->slots_host.data()[(size_t)t * (size_t)e->max_gops + (size_t)slot] = y;
            B->by_ref = true;
            e->frames_by_reference++;
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(dst, y, ny + 2 * nc, kind, ctx->owner->stream));
        }
        B->dev_frames = true;
        B->order.push_back(GopPacket{(uint8_t)type, slot, t});
        e->frames_in++;
        return PFV_OK;
    }
    if (u == y + ny && v == u + nc) {   // a packed frame: one copy
        HIP_TRY(ctx, hipMemcpyAsync(dst, y, ny + 2 * nc, kind, e->copy_stream));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(dst, y, ny, kind, e->copy_stream));
        HIP_TRY(ctx, hipMemcpyAsync(dst + ny, u, nc, kind, e->copy_stream));
        HIP_TRY(ctx, hipMemcpyAsync(dst + ny + nc, v, nc, kind, e->copy_stream));
    }
    B->order.push_back(GopPacket{(uint8_t)type, slot, t});
    e->frames_in++;
    // the caller's planes are free again when the call returns (they are being read by the copy engine until then; the kernels of the
    // previous batch run underneath)
    GopClock clk;
    HIP_TRY(ctx, hipStreamSynchronize(e->copy_stream));
    e->stats[0] += clk.lap();
    return PFV_OK;
}

extern "C" {

PFV_API void pfv_gop_encoder_destroy(pfv_gop_encoder *e)
{
    if (!e) return;
    pfv_ctx *ctx = e->ctx;
    (void)hipSetDevice(ctx->device);
    if (ctx->owner) (void)hipStreamSynchronize(ctx->owner->stream);      // frame copies into the batch buffers
    (void)hipStreamSynchronize(ctx->stream);
    if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
    for (GopEncBatch &B : e->batch) {
        if (B.entries_dev) (void)hipFree(B.entries_dev);
        if (B.frames_dev) (void)hipFree(B.frames_dev);
        if (B.slots_dev) (void)hipFree(B.slots_dev);
        if (B.arena) (void)hipFree(B.arena);
        if (B.cont_save) (void)hipFree(B.cont_save);
        if (B.cursor_dev) (void)hipFree(B.cursor_dev);
        if (B.ev_uploaded) (void)hipEventDestroy(B.ev_uploaded);
        if (B.ev_done) (void)hipEventDestroy(B.ev_done);
        if (B.ev_dev_frames) (void)hipEventDestroy(B.ev_dev_frames);
        for (hipEvent_t ev : B.ev_step) (void)hipEventDestroy(ev);
    }
    if (e->down_stream) { (void)hipStreamSynchronize(e->down_stream); (void)hipStreamDestroy(e->down_stream); }
    if (e->coef) (void)hipFree(e->coef);
    if (e->mv) (void)hipFree(e->mv);
    if (e->has) (void)hipFree(e->has);
    if (e->cursor_host) (void)hipHostFree(e->cursor_host);
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    pfv_enc_session_destroy(e->hot);
    pfv_ctx_destroy(ctx);
    delete e;
}

// Encoder::new (src/enc.rs:37-73) + the batch shape.  max_gops: groups per batch = slots per launch; max_gop_frames: frames a group may
// have inside one batch (a longer run continues in the next batch); payload_budget: bytes of device memory for the packet payloads of
// ONE batch.  0 (default): twice the batch's raw frame bytes (at least 16 MiB) -- real content stays below 1.6 x raw (binary noise at
// quality 0: 1.52 x); a batch that outgrows its arena all the same is encoded again frame by frame (gop_enc_redo) and the arena grows, so like
// Encoder::encode_pframe (src/enc.rs:125-173) the object cannot fail for size.  An explicit budget is kept as given: a batch whose payloads
// exceed it fails with PFV_ERR_NOMEM and the stream stays incomplete (the caller asked for the bound).
PFV_API int pfv_gop_encoder_create(pfv_ctx *ctx, int width, int height, int framerate, int quality, int max_gops, int max_gop_frames,
                                   size_t payload_budget, pfv_gop_encoder **out)
{
    if (!ctx || !out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_gop_encoder_create: bad argument");
    *out = nullptr;
    if (framerate < 0 || framerate > 65535) return fail(ctx, PFV_ERR_BAD_ARG, "framerate must fit u16 (src/enc.rs:197)");
    if (max_gops <= 0 || max_gop_frames <= 0 || max_gops > 4096 || max_gop_frames > 4096)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_gop_encoder_create: max_gops and max_gop_frames must be in 1..4096");
    pfv_ctx *user = ctx;
    int rc = ctx_create_child(user, &ctx);              // from here on `ctx` is the encoder's own launch context (the caller's device and stream priority)
    if (rc) return fail(user, rc, pfv_last_error(nullptr));
    pfv_enc_session *hot = nullptr;
    rc = pfv_enc_session_create(ctx, width, height, quality, max_gops, &hot);
    if (rc) { pfv_ctx_destroy(ctx); return rc; }
    pfv_gop_encoder *e = new pfv_gop_encoder();
    e->ctx = ctx; e->hot = hot; e->width = width; e->height = height; e->max_gops = max_gops; e->max_len = max_gop_frames;
    e->frame_bytes = pfv_frame_bytes(width, height);
    e->total_blocks = (size_t)pfv_total_blocks(width, height);
    const size_t cap_frames = (size_t)max_gops * (size_t)max_gop_frames, nmb = (size_t)max_gops * e->total_blocks;
    // default: twice the batch's raw frame bytes -- real content stays below 1.6 x (binary noise at quality 0: 1.52 x); a batch that outgrows
    // its arena all the same is encoded again frame by frame and the arena grows (gop_enc_redo): the object cannot fail for size.  An explicit
    // budget is kept as given.  PFV_TEST_GOP_ARENA_BYTES (tests only): a default small enough for ordinary content to outgrow.
    e->explicit_budget = payload_budget != 0;
    e->quality = quality;
    e->arena_cap = payload_budget ? payload_budget : std::max<size_t>(2 * cap_frames * e->frame_bytes, (size_t)16 << 20);
    if (!payload_budget && getenv("PFV_TEST_GOP_ARENA_BYTES")) e->arena_cap = std::max<size_t>(64, strtoull(getenv("PFV_TEST_GOP_ARENA_BYTES"), nullptr, 10));
    e->arena_cap = (e->arena_cap + 15) & ~(size_t)15;
    hipError_t he = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->down_stream, hipStreamNonBlocking);
    for (GopEncBatch &B : e->batch) {
        for (int t = 0; t < max_gop_frames && he == hipSuccess; t++) {
            hipEvent_t ev = nullptr;
            he = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (he == hipSuccess) B.ev_step.push_back(ev);
        }
        if (he == hipSuccess && (!B.cursor_steps.resize((size_t)max_gop_frames) || !B.cursor_steps.pinned)) he = hipErrorOutOfMemory;   // k_ent_retain stores to it
        if (he == hipSuccess) he = hipMalloc((void **)&B.frames_dev, cap_frames * e->frame_bytes);
        if (he == hipSuccess) he = hipMalloc((void **)&B.slots_dev, cap_frames * sizeof(const uint8_t *));
        if (he == hipSuccess && (!B.slots_host.resize(cap_frames) || !B.slots_host.pinned)) he = hipErrorOutOfMemory;
        if (he == hipSuccess) { he = hipMalloc((void **)&B.arena, e->arena_cap); B.arena_cap = e->arena_cap; }
        if (he == hipSuccess) he = hipMalloc((void **)&B.entries_dev, cap_frames * sizeof(EntEntry));
        if (he == hipSuccess) he = hipMalloc((void **)&B.cursor_dev, sizeof(unsigned long long));
        if (he == hipSuccess) he = hipEventCreateWithFlags(&B.ev_uploaded, hipEventDisableTiming);
        if (he == hipSuccess) he = hipEventCreateWithFlags(&B.ev_done, hipEventDisableTiming);
        if (he == hipSuccess) he = hipEventCreateWithFlags(&B.ev_dev_frames, hipEventDisableTiming);
    }
    if (he == hipSuccess) he = hipMalloc((void **)&e->coef, nmb * 512);
    if (he == hipSuccess) he = hipMalloc((void **)&e->mv, nmb * 2);
    if (he == hipSuccess) he = hipMalloc((void **)&e->has, nmb);
    if (he == hipSuccess) he = hipHostMalloc((void **)&e->cursor_host, sizeof(unsigned long long), hipHostMallocDefault);
    if (he != hipSuccess) {
        rc = hip_fail(ctx, he, "pfv_gop_encoder_create");
        pfv_gop_encoder_destroy(e);
        return rc;
    }
    rc = pfv_enc_entropy_enable(hot, 0);
    if (!rc && !e->entries_host.resize(cap_frames)) rc = fail(ctx, PFV_ERR_NOMEM, "pinned staging");
    // landing zones for the payloads of a batch: a sixth of its raw bytes (+ 16 KiB) to begin with (quality-5 p-frames of noisy content
    // reach a tenth); they grow on demand
    for (GopEncBatch &B : e->batch)
        if (!rc && !B.payload_host.resize(std::min(e->arena_cap, cap_frames * e->frame_bytes / 6 + ((size_t)16 << 10)))) rc = fail(ctx, PFV_ERR_NOMEM, "pinned payload staging");
    if (rc) { pfv_gop_encoder_destroy(e); return rc; }
    put_header(e->out, width, height, framerate, &quality, 1);
    *out = e;
    return PFV_OK;
}

// Encoder::encode_iframe / encode_pframe / encode_dropframe (src/enc.rs:75-123, 125-173, 175-180).  The planes may be reused as soon
// as the call returns; the packet appears (pfv_gop_encoder_drain) when its batch is complete -- pfv_gop_encoder_flush forces that.
PFV_API int pfv_gop_encoder_encode_iframe(pfv_gop_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v) { return gop_enc_frame(e, 1, y, u, v); }
PFV_API int pfv_gop_encoder_encode_pframe(pfv_gop_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v) { return gop_enc_frame(e, 2, y, u, v); }
// the same for a packed frame (Y | U | V, pfv_frame_bytes) that lies in DEVICE memory -- frames a renderer or another kernel left in HBM:
// nothing crosses PCIe on the way in.  Ordered on the context's stream like every *_dev call: the frame is read behind the work enqueued
// there before the call and may be overwritten by work enqueued there after it (a producer on another stream: pfv_ctx_wait_event).
static int gop_enc_frame_dev(pfv_gop_encoder *e, int type, const uint8_t *frame_dev)
{
    if (!e || !frame_dev) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_gop_encoder_encode_*_dev: bad argument");
    const size_t ny = (size_t)e->width * e->height, nc = (size_t)(e->width / 2) * (e->height / 2);
    return gop_enc_frame(e, type, frame_dev, frame_dev + ny, frame_dev + ny + nc, true);
}
// Frames handed to the *_dev calls are read WHERE THEY LIE instead of being copied into the batch (16-byte aligned frames; others are copied as
// before).  The caller promises that such a frame stays valid and unchanged until its batch has been collected: until the packet of that frame
// has been handed out (pfv_gop_encoder_drain*), or pfv_gop_encoder_flush / _finish has returned.  Same bytes.
PFV_API int pfv_gop_encoder_set_frames_by_reference(pfv_gop_encoder *e, int on)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    e->frames_by_ref = on != 0;
    return PFV_OK;
}
// The motion search of the batches submitted from now on (the hot session's mode; a batch made again takes it too).  Refused while a batch is
// in flight: its frames were searched one way and would be made again the other.
PFV_API int pfv_gop_encoder_set_motion_search(pfv_gop_encoder *e, int mode, int radius)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->batch[0].in_flight || e->batch[1].in_flight) return fail(e->ctx, PFV_ERR_STATE, "pfv_gop_encoder_set_motion_search: a batch is in flight (pfv_gop_encoder_flush first)");
    return pfv_enc_session_set_motion_search(e->hot, mode, radius);
}
PFV_API int pfv_gop_encoder_encode_iframe_dev(pfv_gop_encoder *e, const uint8_t *frame_dev) { return gop_enc_frame_dev(e, 1, frame_dev); }
PFV_API int pfv_gop_encoder_encode_pframe_dev(pfv_gop_encoder *e, const uint8_t *frame_dev) { return gop_enc_frame_dev(e, 2, frame_dev); }
PFV_API int pfv_gop_encoder_encode_dropframe(pfv_gop_encoder *e)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:176)");
    if (e->failed) return fail(e->ctx, PFV_ERR_STATE, "an earlier batch failed: the stream is incomplete");
    e->batch[e->cur].order.push_back(GopPacket{3, 0, 0});
    return PFV_OK;
}
// every frame handed over so far becomes packets now (both batches, in stream order)
PFV_API int pfv_gop_encoder_flush(pfv_gop_encoder *e)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->failed) return fail(e->ctx, PFV_ERR_STATE, "an earlier batch failed: the stream is incomplete");
    pfv_ctx *ctx = e->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = gop_enc_submit(e, e->batch[e->cur]);            // its kernels run while the older batch's payloads come over
    if (!rc) rc = gop_enc_collect(e, e->batch[e->cur ^ 1]);  // packets of the older batch first
    if (!rc) rc = gop_enc_collect(e, e->batch[e->cur]);
    if (rc) e->failed = true;
    return rc;
}
// Encoder::finish (src/enc.rs:182-188)
PFV_API int pfv_gop_encoder_finish(pfv_gop_encoder *e)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:183)");
    int rc = pfv_gop_encoder_flush(e);
    if (rc) return rc;
    e->finished = true;
    e->segs.push_back(pfv_iovec{kPfvEof, sizeof kPfvEof});
    return PFV_OK;
}
PFV_API int pfv_gop_encoder_bytes(pfv_gop_encoder *e, const uint8_t **data, size_t *len)
{
    if (!e || !data || !len) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_gop_encoder_bytes: bad argument");
    gop_enc_materialize(e);
    *data = e->out.data();
    *len = e->out.size();
    return PFV_OK;
}
PFV_API int pfv_gop_encoder_drain(pfv_gop_encoder *e, const uint8_t **data, size_t *len)
{
    if (!e || !data || !len) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_gop_encoder_drain: bad argument");
    gop_enc_materialize(e);
    e->drained.swap(e->out);
    e->out.clear();
    *data = e->drained.data();
    *len = e->drained.size();
    return PFV_OK;
}
// The writer side without a copy (the reference's W: Write takes the packets one write_all at a time, src/enc.rs:190-235): the bytes
// produced since the last drain as `count` segments in stream order -- packet headers, and payloads where the device-to-host copy put
// them (page-locked memory).  Valid until the next call on this encoder.
PFV_API int pfv_gop_encoder_drain_iov(pfv_gop_encoder *e, const pfv_iovec **iov, size_t *count)
{
    if (!e || !iov || !count) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_gop_encoder_drain_iov: bad argument");
    e->segs_drained.clear();
    e->drained.swap(e->out);
    e->out.clear();
    if (!e->drained.empty()) e->segs_drained.push_back(pfv_iovec{e->drained.data(), e->drained.size()});
    e->segs_drained.insert(e->segs_drained.end(), e->segs.begin(), e->segs.end());
    e->segs.clear();
    e->segs_in = 0;
    *iov = e->segs_drained.data();
    *count = e->segs_drained.size();
    return PFV_OK;
}

PFV_API long pfv_gop_encoder_batches(const pfv_gop_encoder *e) { return e ? e->batches : 0; }
/* host seconds so far: out[0] waiting for plane uploads, [1] enqueueing batches, [2] waiting for a batch's kernels, [3] payloads device ->
 * host, [4] packet assembly; returns the number of entries written (<= n) */
PFV_API int pfv_gop_encoder_stats(const pfv_gop_encoder *e, double *out, int n)
{
    if (!e || !out) return 0;
    const int k = std::min(n, 7);
    for (int i = 0; i < k; i++) out[i] = i < 5 ? e->stats[i] : (i == 5 ? (double)e->frames_by_reference : (double)e->batches_redone);
    return k;
}

}  // extern "C"
