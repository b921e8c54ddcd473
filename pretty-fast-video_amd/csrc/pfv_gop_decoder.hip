// pfv_gop_decoder.hip -- pfv_gop_decoder, the GOP-batched stream decoder (the batch model: pfv_gop.hip, whose GopClock and gop_runs it uses).
// Part of the one translation unit of the C ABI: included by pfv_capi.hip behind pfv_gop.hip, never compiled on its own.
#pragma once

struct GopDecEvent {
    enum Kind { FRAME, DROP, END, ERROR } kind = END;
    int rc = 0;                          // ERROR: status; FRAME: parse / decode status (set while the batch is decoded)
    const char *msg = "";
    uint8_t type = 0;                    // FRAME: 1 / 2
    int slot = 0, t = 0;
    const uint8_t *payload = nullptr;
    uint32_t plen = 0;
    size_t pos_after = 0;
};

struct GopDecSet : StepStage {   // host staging of one frame step (kGopDecSets in rotation: steps are parsed under the device work of those before them)
    std::vector<GopDecEvent *> ev;       // per slot: the packet of this step, or null
    hipEvent_t done = nullptr;           // the device has finished reading this set
    bool used = false;
    int pending = 0;                     // parse tasks of this set not yet finished (under the pool's mutex)
};

// staging sets in rotation: the packets of up to kGopDecSets - 1 frame steps are being parsed while the device works on a step, so the
// parser pool always has a few dozen packets to choose from (one step of a 4K stream is 20 packets of ~6 ms: too few for 16 cores
// to stay busy across the step boundaries)
constexpr int kGopDecSets = 4;

// one packet of a batch on the device-entropy path
struct GopDevPacket {
    GopDecEvent *ev = nullptr;
    int rc = 0;                          // status the frame is delivered with (0: decoded)
    bool host_parse = false;             // the host parser reads it (degenerate table, oversize, or the device stage was not sure)
    uint8_t qidx[3] = {0, 0, 0};
    size_t frame = 0;                    // t * max_gops + slot: its place in the batch-wide arrays
};

constexpr int kGopDevDense = 8;

// device-entropy path of the decoder (PFV_OPT_ENTROPY_DECODE): the whole batch's payloads are read by the k_entd_* kernels
struct GopDecDev {
    bool on = false;
    size_t frames_cap = 0;               // max_gops * max_gop_frames
    // the device buffers, BATCH-wide (all packets, one list per frame, no dense arrays; status words on the host with them): a step's window
    // is a view of them (win.bufs() with its packets and workgroups patched in).  Sized up front and grown by this object's own policy; win.done and win.owner are not used.
    DecWindow win;
    size_t pk_cap = 0;                   // packets win.pk_dev / win.status_dev have room for
    std::vector<size_t> list_off;        // per packet: where its list's place (win.list_room entries) starts in the pool
    // the entropy stage's own streams: it works ahead of the decode kernels and their downloads, and the windows take the streams in turn, so
    // that one window's settling tail (a few lanes in a few wavefronts, round after round) runs beside the next windows' full reads.
    // Measured, config 4 with the frames left in HBM (tools/gpu_inner_sweep.sh, three passes each): one stream 1.25-1.27 G macroblocks/s at
    // the device's greatest stream priority (1.22-1.29 without), two / three streams 1.12-1.24 / 1.16-1.25 (0.89-1.10 without priority: the
    // decode launches then wait behind them), four streams at normal priority 1.27-1.40.  Re-measured at the end of round 5 on one box, passes
    // interleaved (tools/e2e_native.cpp; PFV_GOPD_WINDOW_STREAMS): four 1.14-1.18 G, THREE 1.27-1.34, two 1.03-1.05; the Python probe's wait for
    // the entropy stage 8.0-8.6 / 6.9-7.4 / 9.5-9.7 ms.  (The runtime multiplexes a process's streams over four hardware queues; with the context's
    // stream and the upload stream four window streams make six.  The upload stream at the greatest priority -- a queue pool of its own -- also
    // gave 1.21-1.24 with four; the two together nothing more.)
    static constexpr int kStreams = 4;
    hipStream_t streams[kStreams] = {nullptr, nullptr, nullptr, nullptr};
    int n_streams = 3;
    hipStream_t up_stream = nullptr;     // ... and the uploads / clears it needs run ahead of it on a third
    std::vector<hipEvent_t> window_done; // per step: payloads read, statuses on the host
    std::vector<hipEvent_t> window_up;   // per step: payloads, headers and cleared coefficient arrays in place
    PinnedBuf<uint8_t> bytes_host, has_host;
    PinnedBuf<int8_t> mv_host;
    PinnedBuf<EdPacket> pk_host;
    PinnedBuf<uint2> groups_host;
    uint32_t sub_bits = kEdSubBits;      // payload bits per lane (PFV_OPT_ENTDEC_LANE_BITS)
    int launches = 3, inner = kEdInner;  // read launches before the verifying one (k_entd_sync + launches - 1 x k_entd_fix), rounds inside the first (PFV_OPT_ENTDEC_LAUNCHES / _INNER_ROUNDS)
    long unsettled = 0, irregular = 0;   // why packets were left to the host parser
    PinnedBuf<uint32_t> hp_ent;          // up to kGopDevDense packets the host parser reads, in list form: entries (a packet's share: its place's size) ...
    PinnedBuf<uint32_t> hp_counts;       // ... and counts [kGopDevDense][tb + 1]
    PinnedBuf<uint32_t> hp_full;         // one packet whose list outgrew its place (tb x 256 entries)
    size_t hp_off[kGopDevDense] = {}, hp_n[kGopDevDense] = {};
    std::vector<GopDevPacket> pk;
    std::vector<int> todo;               // phase 2: the packets the host parser reads, kGopDevDense at a time
    int todo_first = 0;
    int pending = 0;                     // phase-2 tasks (packets parsed on the host) not yet finished (under the pool's mutex)
    std::vector<int> step_pending;       // phase-1 tasks (headers) not yet finished, per frame step
    long packets_dev = 0, packets_host = 0, batches_dev = 0, batches_host = 0;
};

struct pfv_gop_decoder {
    pfv_ctx *ctx = nullptr;
    pfv_dec_session *hot = nullptr;
    GopDecDev dev;
    const uint8_t *data = nullptr;
    size_t len = 0, pos = 0, reset_pos = 0;
    int width = 0, height = 0, framerate = 0, n_qtables = 0, max_gops = 0, max_len = 0;
    size_t total_blocks = 0, frame_bytes = 0, cap = 0;
    bool eof = false;
    double delta_accum = 0.0;
    // the current batch
    std::vector<GopDecEvent> events;     // stream order
    size_t next_event = 0;
    std::vector<int> glen;               // frames per group
    std::vector<uint8_t> gfirst;         // type of the group's first frame
    bool cont_valid = false;
    int cont_buf = 0, cont_slot = 0;     // where the framebuffer of the previous batch's last group lives (buffer, slot)
    GopDecSet set[kGopDecSets];
    PinnedBuf<int16_t> dense;            // one slot's coefficients when its list overflowed
    PinnedBuf<uint8_t> frames_host;      // [max_gop_frames][max_gops][frame_bytes]: the decoded frames of the batch
    PinnedBuf<int> flags;                // [step][max_gops]: bad-motion-vector flags of the batch's steps, attributed when the batch is closed
    uint8_t *frames_dev = nullptr;       // [max_gops][frame_bytes]
    bool out_dev = false;                // pfv_gop_decoder_set_output_device: frames stay in HBM, the callback gets device pointers
    uint8_t *frames_all_dev = nullptr;   // [steps][max_gops][frame_bytes] then
    size_t frames_all_cap = 0;           // bytes
    long batches = 0, dense_packets = 0;
    // seconds: [0] header scan, [1] waiting for packet parsers (the caller parses too), [2] waiting for the device before a staging set
    // can be reused, [3] enqueueing, [4] waiting for the batch's last frames
    double stats[6] = {0, 0, 0, 0, 0, 0};   // [5]: waiting for the device's entropy stage (device-entropy path)
    // worker pool: the packets of a step are parsed in parallel (one task per slot)
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    std::deque<std::pair<GopDecSet *, int>> tasks;   // (staging set, slot) packets waiting for a parser
    bool quit = false;
};

static void gopd_parse_one(pfv_gop_decoder *d, GopDecSet *s, int k)   // only slots with a packet are queued (gopd_start_parse)
{
    const GopDecEvent *e = s->ev[(size_t)k];
    s->parse(k, e->type, e->payload, e->plen, d->total_blocks, d->n_qtables, d->cap);
}
static void gopd_dev_task(pfv_gop_decoder *d, int j);
// a queued task: (staging set, slot) = parse that packet into the set's lists; (null, j >= 0) = the headers of packet j of the device-entropy
// path's batch (phase 1); (null, -1 - j) = the j-th packet of the current group the device stage left to the host parser (phase 2)
static void gopd_run_task(pfv_gop_decoder *d, const std::pair<GopDecSet *, int> &job)
{
    if (job.first) gopd_parse_one(d, job.first, job.second);
    else gopd_dev_task(d, job.second);
}
// a task has been run (or dropped): its counters, under the pool's mutex.  Device-path tasks count per phase and, in phase 1 (headers), per frame
// step as well: the windows of a step are enqueued as soon as ITS packets are ready.  True when some waiter may go on.
static bool gopd_task_done(pfv_gop_decoder *d, const std::pair<GopDecSet *, int> &job)
{
    if (job.first) return --job.first->pending == 0;
    GopDecDev &v = d->dev;
    if (job.second < 0) return --v.pending == 0;        // a packet parsed on the host (phase 2)
    return --v.step_pending[(size_t)v.pk[(size_t)job.second].ev->t] == 0;
}
static void gopd_worker(pfv_gop_decoder *d)
{
    std::unique_lock<std::mutex> lk(d->m);
    for (;;) {
        d->cv_work.wait(lk, [&] { return d->quit || !d->tasks.empty(); });
        if (d->quit) return;
        const auto job = d->tasks.front();
        d->tasks.pop_front();
        lk.unlock();
        gopd_run_task(d, job);
        lk.lock();
        if (gopd_task_done(d, job)) d->cv_done.notify_all();
    }
}
static void gopd_start_parse(pfv_gop_decoder *d, GopDecSet *s, int n_slots)
{
    std::lock_guard<std::mutex> lk(d->m);
    for (int k = 0; k < n_slots; k++) {
        s->counts.data()[k] = 0;
        s->rc[(size_t)k] = 0;
        if (s->ev[(size_t)k]) { d->tasks.emplace_back(s, k); s->pending++; }
    }
    d->cv_work.notify_all();
}
static void gopd_join(pfv_gop_decoder *d, int *pending)
{
    std::unique_lock<std::mutex> lk(d->m);
    while (*pending > 0) {
        if (!d->tasks.empty()) {     // the caller parses too (and is the whole pool when there are no workers): any packet will do
            const auto job = d->tasks.front();
            d->tasks.pop_front();
            lk.unlock();
            gopd_run_task(d, job);
            lk.lock();
            if (gopd_task_done(d, job)) d->cv_done.notify_all();
        } else {
            d->cv_done.wait(lk);
        }
    }
}
static void gopd_join_parse(pfv_gop_decoder *d, GopDecSet *s) { gopd_join(d, &s->pending); }
// nothing of an abandoned batch may stay queued (reset, errors): wait for the parsers to let go of the sets
static void gopd_drain_pool(pfv_gop_decoder *d)
{
    std::unique_lock<std::mutex> lk(d->m);
    for (const auto &job : d->tasks) (void)gopd_task_done(d, job);
    d->tasks.clear();
    d->cv_done.wait(lk, [&] {
        for (const GopDecSet &s : d->set)
            if (s.pending > 0) return false;
        for (int p : d->dev.step_pending)
            if (p > 0) return false;
        return d->dev.pending <= 0;
    });
}

// Walks the packet headers from d->pos exactly as the reference's loop does (src/dec.rs:174-222) and cuts the next batch: up to
// max_gops groups of up to max_gop_frames frame packets, a group per i-frame.
static void gopd_scan_batch(pfv_gop_decoder *d)
{
    d->events.clear(); d->next_event = 0; d->glen.clear(); d->gfirst.clear();
    size_t pos = d->pos;
    auto push = [&](GopDecEvent::Kind kind, size_t pos_after) -> GopDecEvent & {
        d->events.emplace_back();
        GopDecEvent &e = d->events.back();
        e.kind = kind; e.pos_after = pos_after;
        return e;
    };
    for (;;) {
        PfvPacket pk;
        const int rc = next_packet(d->data, d->len, pos, pk);
        if (rc || pk.type == 0) {   // the stream ends here, as it should (EOF marker, :183-187) or not
            GopDecEvent &e = push(rc ? GopDecEvent::ERROR : GopDecEvent::END, pk.pos_after);
            e.rc = rc; e.msg = pk.msg;
            break;
        }
        const uint8_t type = pk.type;
        const uint32_t plen = pk.plen;
        const size_t after = pk.pos_after;
        if (type != 1 && type != 2) { pos = after; continue; }                      // unknown packet: skipped (:216-219)
        if (type == 1 && plen == 0) { push(GopDecEvent::DROP, after); pos = after; continue; }   // drop frame (:190)
        if (type == 1) {
            if ((int)d->glen.size() == d->max_gops) break;                          // the next batch starts here
            d->glen.push_back(0); d->gfirst.push_back(1);
        } else if (d->glen.empty() || d->glen.back() == d->max_len) {
            if (!d->glen.empty()) break;                                            // a run longer than a batch holds: it continues in the next one
            d->glen.push_back(0); d->gfirst.push_back(2);
        }
        GopDecEvent &e = push(GopDecEvent::FRAME, after);
        e.type = type; e.payload = pk.payload; e.plen = plen;
        e.slot = (int)d->glen.size() - 1; e.t = d->glen.back()++;
        pos = after;
    }
}

// where a batch's frames go: page-locked host memory [step][slot] (the default), or a device array of the same shape; the steps' bad-vector
// flags, cleared, beside them.  Merged chains (gopd_decode_batch) make `steps` exceed max_gop_frames.
static int gopd_out_room(pfv_gop_decoder *d, int steps)
{
    pfv_ctx *ctx = d->ctx;
    const size_t places = (size_t)std::max(steps, 1) * (size_t)d->max_gops, need = places * d->frame_bytes;
    if (!d->flags.resize(places)) return fail(ctx, PFV_ERR_NOMEM, "pinned flag staging");
    memset(d->flags.data(), 0, places * sizeof(int));
    if (!d->out_dev) return d->frames_host.resize(need) ? PFV_OK : fail(ctx, PFV_ERR_NOMEM, "pinned frame staging");
    if (need <= d->frames_all_cap) return PFV_OK;
    if (d->frames_all_dev) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(d->frames_all_dev); d->frames_all_dev = nullptr; d->frames_all_cap = 0; }
    HIP_TRY(ctx, hipMalloc((void **)&d->frames_all_dev, need));
    d->frames_all_cap = need;
    return PFV_OK;
}
// the retframes of step t, slots [first, first + count), after dec_launch: the separate crop pass where the fused one does not apply, and
// the way to the host
static int gopd_step_out(pfv_gop_decoder *d, int t, int first, int count)
{
    pfv_ctx *ctx = d->ctx;
    pfv_dec_session *hot = d->hot;
    int rc = PFV_OK;
    if (!fused_output_ok(hot)) {             // geometries without 16-byte rows: on the buffer just written
        hot->cur ^= 1;
        rc = dec_crop_win(hot, first, count, hot->frames_out, 0);
        hot->cur ^= 1;
    }
    if (!rc && !d->out_dev &&
        hipMemcpyAsync(d->frames_host.data() + ((size_t)t * (size_t)d->max_gops + (size_t)first) * d->frame_bytes, d->frames_dev + (size_t)first * d->frame_bytes,
                       (size_t)count * d->frame_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(ctx, PFV_ERR_HIP, "retframe download");
    return rc;
}

// ---------------------------------------------------------------- what a frame step is, whichever side read its packets
static const char *const kGopdBadPayload = "malformed packet payload";
static const char *const kGopdBadMv = "motion vector points outside the reference plane (src/common.rs:258-259)";

// slot 0 continues the run the previous batch left open: that run's last frame becomes its reference
static int gopd_continue_run(pfv_gop_decoder *d, bool head_continues)
{
    pfv_dec_session *hot = d->hot;
    if (!head_continues || !d->cont_valid) return PFV_OK;
    const size_t pad = (size_t)hot->geom.pad_frame_bytes;
    const uint8_t *src = hot->fb[d->cont_buf] + (size_t)d->cont_slot * pad;
    uint8_t *dst = hot->fb[hot->cur];
    if (src != dst) HIP_TRY(d->ctx, hipMemcpyAsync(dst, src, pad, hipMemcpyDeviceToDevice, d->ctx->stream));
    return PFV_OK;
}
// A failed packet changes nothing (its error surfaces when the frame is delivered), but its slot's framebuffer has to follow the ping-pong
// for the frames behind it.
static int gopd_hold_slot(pfv_gop_decoder *d, int k)
{
    pfv_dec_session *hot = d->hot;
    const size_t pad = (size_t)hot->geom.pad_frame_bytes;
    HIP_TRY(d->ctx, hipMemcpyAsync(hot->fb[hot->cur ^ 1] + (size_t)k * pad, hot->fb[hot->cur] + (size_t)k * pad, pad, hipMemcpyDeviceToDevice, d->ctx->stream));
    return PFV_OK;
}
static bool gopd_qidx_ok(const pfv_dec_session *hot, const uint8_t q[3])   // the reference panics (src/dec.rs:249-251)
{
    return q[0] < hot->n_qtables && q[1] < hot->n_qtables && q[2] < hot->n_qtables;
}
// launch key of a packet that runs: its (frame type, q-table indices) among the distinct ones of the step
static int gopd_key(std::vector<uint32_t> &combos, uint8_t type, const uint8_t q[3])
{
    const uint32_t c = (uint32_t)type | ((uint32_t)q[0] << 8) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 24);
    size_t ci = 0;
    while (ci < combos.size() && combos[ci] != c) ci++;
    if (ci == combos.size()) combos.push_back(c);
    return (int)ci;
}
// Step t once its inputs are on their way: a launch per run of neighbouring slots of one key (key[k] < 0: slot k sits the step out) with the
// frames' way out behind it, the ping-pong flip, the step's bad-vector flags into the batch-wide array
static int gopd_launch_step(pfv_gop_decoder *d, int t, const std::vector<int> &key, const std::vector<uint32_t> &combos, const int8_t *mv, const uint8_t *has,
                            const DecCoefs &coefs)
{
    pfv_ctx *ctx = d->ctx;
    pfv_dec_session *hot = d->hot;
    const size_t place0 = (size_t)t * (size_t)d->max_gops;
    int rc = PFV_OK;
    hot->frames_out = d->out_dev ? d->frames_all_dev + place0 * d->frame_bytes : d->frames_dev;
    gop_runs(key, [&](int first, int count, int ci) {
        if (rc) return;
        const uint32_t c = combos[(size_t)ci];
        const uint8_t q[3] = {(uint8_t)(c >> 8), (uint8_t)(c >> 16), (uint8_t)(c >> 24)};
        rc = dec_launch(hot, (c & 0xffu) == 2, first, count, mv, has, coefs, q);
        if (!rc) rc = gopd_step_out(d, t, first, count);
    });
    if (rc) return rc;
    hot->cur ^= 1;
    HIP_TRY(ctx, hipMemcpyAsync(d->flags.data() + place0, hot->flag_dev, key.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(hot->flag_dev, 0, key.size() * sizeof(int), ctx->stream));
    return PFV_OK;
}
// The batch's last step has been waited for: the bad vectors the kernels flagged go to their frames' events; the run of the last group (slot
// last_root, last_len steps) may go on in the next batch -- its framebuffer is in the buffer its last step wrote.
static void gopd_close_batch(pfv_gop_decoder *d, int cur0, int last_root, int last_len)
{
    for (GopDecEvent &e : d->events)
        if (e.kind == GopDecEvent::FRAME && !e.rc && d->flags.data()[(size_t)e.t * (size_t)d->max_gops + (size_t)e.slot]) { e.rc = PFV_ERR_BAD_MV; e.msg = kGopdBadMv; }
    d->cont_valid = true;
    d->cont_slot = last_root;
    d->cont_buf = (cur0 + last_len) & 1;
    d->batches++;
}

// decode every frame packet of the scanned batch; the frames land in frames_host[step][slot]
static int gopd_decode_batch(pfv_gop_decoder *d)
{
    pfv_ctx *ctx = d->ctx;
    pfv_dec_session *hot = d->hot;
    const int G = (int)d->glen.size();
    if (G == 0) return PFV_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t tb = d->total_blocks;

    // chains: the frame packets a slot decodes one after the other.  To begin with, chain k = group k.
    std::vector<std::vector<GopDecEvent *>> chain((size_t)G);
    for (GopDecEvent &e : d->events)
        if (e.kind == GopDecEvent::FRAME) { e.rc = 0; chain[(size_t)e.slot].push_back(&e); }
    auto wait_set = [&](GopDecSet &s) -> int {   // the device may still be reading the set's lists
        if (!s.used) return PFV_OK;
        GopClock wclk;
        HIP_TRY(ctx, hipEventSynchronize(s.done));
        d->stats[2] += wclk.lap();
        s.used = false;
        return PFV_OK;
    };
    auto fill = [&](GopDecSet &s, int t) {
        for (int k = 0; k < G; k++) s.ev[(size_t)k] = (int)chain[(size_t)k].size() > t ? chain[(size_t)k][(size_t)t] : nullptr;
    };
    // status of a parsed packet: 0 (kSinkFull counts: it is parsed again into the dense form) or the error it is delivered with
    auto status = [&](const GopDecSet &s, int k) -> int {
        const int prc = s.rc[(size_t)k] == kSinkFull ? 0 : s.rc[(size_t)k];
        return !prc && !gopd_qidx_ok(hot, &s.qidx[(size_t)k * 3]) ? PFV_ERR_FORMAT : prc;
    };
    int rc = PFV_OK;
    for (GopDecSet &s : d->set)
        if (!rc) rc = wait_set(s);
    if (rc) return rc;

    // step 0 is parsed before anything runs: a group whose i-frame does not parse is no independent run -- the sequential loop
    // leaves the framebuffer alone and applies the group's p-frames to what the PREVIOUS group left (src/dec.rs:188-214).  Such a
    // group is appended to the chain of the slot before it (slot 0: it continues the run of the previous batch).
    GopClock clk;
    fill(d->set[0], 0);
    gopd_start_parse(d, &d->set[0], G);
    // The steps behind it go to the parsers at the same time, on the assumption that every group's first frame is sound (the i-frames of
    // step 0 are several times the size of a p-frame: without this the pool idles while the slowest of them is read).  If one is not,
    // the chains change and these steps are parsed again.
    int prefilled = 1;
    {
        int steps0 = 0;
        for (int k = 0; k < G; k++) steps0 = std::max(steps0, (int)chain[(size_t)k].size());
        for (int t = 1; t < kGopDecSets && t < steps0; t++) {
            fill(d->set[t], t);
            gopd_start_parse(d, &d->set[t], G);
            prefilled = t + 1;
        }
    }
    gopd_join_parse(d, &d->set[0]);
    // An i-frame whose list overflowed (denser than 1 non-zero in 4) was not read to its end: whether it parses is only known after a
    // full pass, and the chains below depend on it -- read it once more with a sink that keeps nothing (dense i-frames only: rare)
    for (int k = 0; k < G; k++) {
        GopDecEvent *e0 = d->set[0].ev[(size_t)k];
        if (!e0 || e0->type != 1 || d->set[0].rc[(size_t)k] != kSinkFull) continue;
        struct { bool put(size_t, int16_t) { return true; } bool put_if(bool, size_t, int16_t) { return true; } } none;
        uint8_t q[3];
        const int vrc = parse_iframe_to(e0->payload, e0->plen, (int)tb, d->n_qtables, none, q);
        if (vrc) d->set[0].rc[(size_t)k] = vrc;
    }
    d->stats[1] += clk.lap();
    bool reparse = false, head_continues = d->gfirst[0] == 2;
    int last_root = G - 1;
    {
        std::vector<int> root((size_t)G);
        for (int k = 0; k < G; k++) {
            root[(size_t)k] = k;
            GopDecEvent *e0 = chain[(size_t)k].empty() ? nullptr : chain[(size_t)k][0];
            if (!e0 || e0->type != 1) continue;
            const int prc = status(d->set[0], k);
            if (!prc) continue;
            e0->rc = prc; e0->msg = kGopdBadPayload;
            reparse = true;
            const int r = k == 0 ? 0 : root[(size_t)k - 1];
            root[(size_t)k] = r;
            std::vector<GopDecEvent *> rest(chain[(size_t)k].begin() + 1, chain[(size_t)k].end());
            if (k == 0) { chain[0] = rest; head_continues = true; }
            else { chain[(size_t)k].clear(); chain[(size_t)r].insert(chain[(size_t)r].end(), rest.begin(), rest.end()); }
        }
        last_root = root[(size_t)G - 1];
    }
    int steps = 0;
    for (int k = 0; k < G; k++) {
        steps = std::max(steps, (int)chain[(size_t)k].size());
        for (size_t t = 0; t < chain[(size_t)k].size(); t++) { chain[(size_t)k][t]->slot = k; chain[(size_t)k][t]->t = (int)t; }
    }
    if ((rc = gopd_continue_run(d, head_continues))) return rc;
    if ((rc = gopd_out_room(d, steps))) return rc;       // merged chains may be longer than a group
    const int cur0 = hot->cur;
    // steps [t, next_fill) are parsed or being parsed; step s uses staging set s % kGopDecSets.  A set is refilled as soon as the device
    // has finished with the step that used it last.
    if (reparse) gopd_drain_pool(d);         // the chains moved: what was parsed ahead belongs to other (slot, step) places now
    int next_fill = reparse ? 0 : prefilled;
    auto top_up = [&](int t, bool must_have_t) -> int {
        while (next_fill < steps && next_fill < t + kGopDecSets) {
            GopDecSet &n = d->set[next_fill % kGopDecSets];
            if (n.used && !(must_have_t && next_fill <= t) && hipEventQuery(n.done) != hipSuccess) { (void)hipGetLastError(); break; }
            const int wrc = wait_set(n);
            if (wrc) return wrc;
            fill(n, next_fill);
            gopd_start_parse(d, &n, G);
            next_fill++;
        }
        return PFV_OK;
    };
    std::vector<int> key((size_t)G);
    std::vector<uint32_t> combos;            // distinct (frame type, q-table indices) of a step -> launch key
    for (int t = 0; t < steps; t++) {
        GopDecSet &s = d->set[t % kGopDecSets];
        clk.lap();
        if ((rc = top_up(t, true))) return rc;
        d->stats[3] += clk.lap();
        gopd_join_parse(d, &s);
        d->stats[1] += clk.lap();
        // what runs: the packets that parsed
        bool any_dense = false;
        combos.clear();
        for (int k = 0; k < G; k++) {
            GopDecEvent *e = s.ev[(size_t)k];
            key[(size_t)k] = -1;
            if (!e) continue;
            const int prc = status(s, k);
            if (prc) {
                e->rc = prc; e->msg = kGopdBadPayload;
                if ((rc = gopd_hold_slot(d, k))) return rc;
                continue;
            }
            any_dense = any_dense || s.rc[(size_t)k] == kSinkFull;
            key[(size_t)k] = gopd_key(combos, e->type, &s.qidx[(size_t)k * 3]);
        }
        if ((rc = s.scatter(ctx, hot, (size_t)G, tb, d->cap))) return rc;
        if (any_dense) {   // a list overflowed (denser than 1 non-zero in 4): that packet again, into the dense form, on this thread
            for (int k = 0; k < G; k++) {
                GopDecEvent *e = s.ev[(size_t)k];
                if (!e || s.rc[(size_t)k] != kSinkFull || key[(size_t)k] < 0) continue;
                d->dense_packets++;
                if (!d->dense.resize(tb * 256)) return fail(ctx, PFV_ERR_NOMEM, "pinned dense staging");
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));        // the previous user of the dense buffer
                memset(d->dense.data(), 0, tb * 512);
                DenseSink sink{d->dense.data()};
                uint8_t q[3];
                const int prc = parse_frame_to(e->type, e->payload, e->plen, (int)tb, d->n_qtables, s.mv.data() + (size_t)k * tb * 2, s.has.data() + (size_t)k * tb, sink, q);
                if (prc) {
                    e->rc = prc; e->msg = kGopdBadPayload; key[(size_t)k] = -1;
                    if ((rc = gopd_hold_slot(d, k))) return rc;
                    continue;
                }
                HIP_TRY(ctx, hipMemcpyAsync(hot->st_coef + (size_t)k * tb * 256, d->dense.data(), tb * 512, hipMemcpyHostToDevice, ctx->stream));
            }
        }
        HIP_TRY(ctx, hipMemcpyAsync(hot->st_mv, s.mv.data(), (size_t)G * tb * 2, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(hot->st_has, s.has.data(), (size_t)G * tb, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = gopd_launch_step(d, t, key, combos, hot->st_mv, hot->st_has, hot->st_coef))) return rc;
        HIP_TRY(ctx, hipEventRecord(s.done, ctx->stream));
        s.used = true;
        if ((rc = top_up(t + 1, false))) return rc;
        d->stats[3] += clk.lap();
    }
    clk.lap();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    d->stats[4] += clk.lap();
    gopd_close_batch(d, cur0, last_root, (int)chain[(size_t)last_root].size());
    return PFV_OK;
}

// ---------------------------------------------------------------- device-entropy path (PFV_OPT_ENTROPY_DECODE)
// phase 1, per packet: what the kernels need that only a serial read can give -- the table (-> the tree's codes), the q indices, a
// p-frame's block headers (-> motion vectors, has_coeff, the first bit of the run streams); the payload goes to page-locked staging
static void gopd_dev_prepare(pfv_gop_decoder *d, int j)
{
    GopDecDev &v = d->dev;
    GopDevPacket &p = v.pk[(size_t)j];
    const GopDecEvent *e = p.ev;
    EdPacket &k = v.pk_host.data()[j];
    const size_t tb = d->total_blocks;
    const EntdPrep r = entd_prepare(e->payload, e->plen, e->type, tb, d->n_qtables, v.sub_bits, k, v.bytes_host.data() + k.byte_off);
    p.rc = r.rc;
    p.host_parse = r.host_parse;
    memcpy(p.qidx, r.qidx, 3);
}
// phase 2, per packet the device stage left to the host: the host parser, into a dense frame
static void gopd_dev_hostparse(pfv_gop_decoder *d, int j)
{
    GopDecDev &v = d->dev;
    GopDevPacket &p = v.pk[(size_t)v.todo[(size_t)(v.todo_first + j)]];
    const GopDecEvent *e = p.ev;
    const size_t tb = d->total_blocks, pj = (size_t)v.todo[(size_t)(v.todo_first + j)];
    uint8_t q[3];
    p.rc = parse_to_lists(e->payload, e->plen, e->type, tb, d->n_qtables, v.mv_host.data() + p.frame * tb * 2, v.has_host.data() + p.frame * tb, v.hp_ent.data() + v.hp_off[j],
                          v.win.list_room[pj], v.hp_counts.data() + (size_t)j * (tb + 1), &v.hp_n[j], q);
}
static void gopd_dev_task(pfv_gop_decoder *d, int code)
{
    if (code >= 0) gopd_dev_prepare(d, code);
    else gopd_dev_hostparse(d, -1 - code);
}
// phase 2: n_tasks packets (v.todo from todo_first on) through the host parser, on the pool and this thread
static void gopd_dev_hostparse_group(pfv_gop_decoder *d, int n_tasks)
{
    {
        std::lock_guard<std::mutex> lk(d->m);
        for (int j = 0; j < n_tasks; j++) { d->tasks.emplace_front(nullptr, -1 - j); d->dev.pending++; }   // ahead of the headers still queued: a step is waiting
        d->cv_work.notify_all();
    }
    gopd_join(d, &d->dev.pending);
}
// a p-frame packet the HOST parser read: its block headers go up with its lists (the device's own read of them is not what is decoded)
static int gopd_dev_upload_headers(pfv_gop_decoder *d, const GopDevPacket &p)
{
    pfv_ctx *ctx = d->ctx;
    GopDecDev &v = d->dev;
    const size_t tb = d->total_blocks;
    if (p.ev->type != 2) return PFV_OK;
    HIP_TRY(ctx, hipMemcpyAsync(v.win.mv_dev + p.frame * tb * 2, v.mv_host.data() + p.frame * tb * 2, tb * 2, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(v.win.has_dev + p.frame * tb, v.has_host.data() + p.frame * tb, tb, hipMemcpyHostToDevice, ctx->stream));
    return PFV_OK;
}

// Decode the scanned batch with the payloads read on the device.  PFV_OK: done (frames in frames_host[step][slot]); 1: this batch needs
// the host path (a group's i-frame does not parse: the chains change, see gopd_decode_batch) -- nothing has been decoded; negative: error.
//
// The entropy stage of step t (payload upload, k_entd_*, status download) runs on a stream of its own, one window per step, all windows
// enqueued up front: while the context's stream decodes step t and sends its frames to the host -- the PCIe time that bounds the whole
// decoder -- the device reads the payloads of the steps behind it.
static int gopd_decode_batch_dev(pfv_gop_decoder *d)
{
    pfv_ctx *ctx = d->ctx;
    pfv_dec_session *hot = d->hot;
    GopDecDev &v = d->dev;
    DecWindow &w = v.win;
    const int G = (int)d->glen.size();
    if (G == 0) return PFV_OK;
    int steps = 0;
    for (int k = 0; k < G; k++) steps = std::max(steps, d->glen[(size_t)k]);
    if (steps > d->max_len || G > d->max_gops) return 1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t tb = d->total_blocks, S = (size_t)d->max_gops;
    GopClock clk;
    HIP_TRY(ctx, hipStreamSynchronize(v.up_stream));       // a batch that went to the host path may have left windows behind
    for (int k = 0; k < v.n_streams; k++) HIP_TRY(ctx, hipStreamSynchronize(v.streams[k]));

    // packets in (step, slot) order: a step's packets, payload bytes, subsequences and workgroups are contiguous
    v.pk.clear();
    for (GopDecEvent &e : d->events)
        if (e.kind == GopDecEvent::FRAME) {
            GopDevPacket p;
            p.ev = &e;
            p.frame = (size_t)e.t * S + (size_t)e.slot;
            v.pk.push_back(p);
        }
    std::sort(v.pk.begin(), v.pk.end(), [](const GopDevPacket &a, const GopDevPacket &b) { return a.frame < b.frame; });
    const size_t n = v.pk.size();
    if (!v.pk_host.resize(n) || !w.status_host.resize(n)) return fail(ctx, PFV_ERR_NOMEM, "device-entropy staging");
    std::vector<size_t> p0((size_t)steps + 1, n), byte0((size_t)steps + 1, 0);
    size_t bytes_total = 0;
    for (size_t j = 0; j < n; j++) {
        EdPacket &k = v.pk_host.data()[j];
        const size_t t = (size_t)v.pk[j].ev->t;
        if (p0[t] == n) { p0[t] = j; byte0[t] = bytes_total; }
        k.byte_off = bytes_total;
        k.frame_off = v.pk[j].frame;
        bytes_total += ((size_t)v.pk[j].ev->plen + 16 + 15) & ~(size_t)15;
    }
    byte0[(size_t)steps] = bytes_total;
    for (size_t t = (size_t)steps; t-- > 0;)
        if (p0[t] == n) { p0[t] = p0[t + 1]; byte0[t] = byte0[t + 1]; }
    if (!v.bytes_host.resize(bytes_total + 64)) return fail(ctx, PFV_ERR_NOMEM, "device-entropy payload staging");
    // room on the device from upper bounds (a lane per sub_bits payload bits), so that nothing has to wait for the headers
    size_t sub_max = 0, grp_max = 0;
    for (size_t j = 0; j < n; j++) {
        const size_t lanes = ((size_t)v.pk[j].ev->plen * 8 + v.sub_bits - 1) / v.sub_bits;
        sub_max += lanes;
        grp_max += (lanes + kEdOwn - 1) / kEdOwn;
    }
    if (sub_max >= 0xffffffffull) return 1;
    int rc = PFV_OK;
    if (!v.groups_host.resize(std::max<size_t>(grp_max, 1))) return fail(ctx, PFV_ERR_NOMEM, "device-entropy staging");
    if ((rc = dev_room(ctx, &w.bytes_dev, &w.bytes_cap, bytes_total + 64, 4, &ctx->stream))) return rc;
    if (n > v.pk_cap) {
        if (w.pk_dev) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(w.pk_dev); (void)hipFree(w.status_dev); w.pk_dev = nullptr; w.status_dev = nullptr; v.pk_cap = 0; }
        HIP_TRY(ctx, hipMalloc((void **)&w.pk_dev, (n + n / 4) * sizeof(EdPacket)));
        HIP_TRY(ctx, hipMalloc((void **)&w.status_dev, (n + n / 4) * sizeof(uint32_t)));
        v.pk_cap = n + n / 4;
    }
    if ((rc = dev_room(ctx, &w.groups_dev, &w.groups_cap, std::max<size_t>(grp_max, 1), 4, &ctx->stream))) return rc;
    if ((rc = dev_room(ctx, &w.sub_dev, &w.sub_cap, std::max<size_t>(sub_max, 1) * 4, 4, &ctx->stream))) return rc;
    if ((rc = dev_room(ctx, &w.wgsum_dev, &w.wgsum_cap, std::max<size_t>(grp_max, 1), 4, &ctx->stream))) return rc;
    size_t hdr_max = 0;
    for (size_t j = 0; j < n; j++) hdr_max += v.pk[j].ev->type == 2 ? entd_hdr_wgs(tb, v.pk[j].ev->plen) : 0;
    if ((rc = dev_room(ctx, &w.hdr_maps_dev, &w.hdr_maps_cap, (hdr_max + 1) * 8, 4, &ctx->stream))) return rc;
    if ((rc = dev_room(ctx, &w.hdr_start_dev, &w.hdr_start_cap, hdr_max + 1, 4, &ctx->stream))) return rc;
    // the coefficient lists: every packet's place in the pool from its size alone (entd_pool_cap), the frames' list pointers with them
    v.list_off.assign(n, 0); w.list_room.assign(n, 0);
    size_t list_total = 0;
    for (size_t j = 0; j < n; j++) {
        v.list_off[j] = list_total;
        w.list_room[j] = entd_pool_cap(tb, v.pk[j].ev->plen);
        list_total += w.list_room[j];
    }
    if (list_total > w.lists.ent_cap) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // the previous batch's decode launches read the pool
    w.lists.drop_spill();                                                                     // (ctx->stream is idle between batches: the frames were waited for)
    if ((rc = w.lists.room(ctx, std::max<size_t>(list_total, 4)))) return rc;
    for (size_t f = 0; f < v.frames_cap; f++) w.lists.ptr_host.data()[f] = nullptr;
    for (size_t j = 0; j < n; j++) w.lists.ptr_host.data()[v.pk[j].frame] = w.lists.ent + v.list_off[j];
    HIP_TRY(ctx, hipMemcpyAsync(w.lists.ptr_dev, w.lists.ptr_host.data(), v.frames_cap * sizeof(uint32_t *), hipMemcpyHostToDevice, v.up_stream));
    while (v.window_done.size() < (size_t)steps) {
        hipEvent_t ev = nullptr, ev2 = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        v.window_done.push_back(ev);
        HIP_TRY(ctx, hipEventCreateWithFlags(&ev2, hipEventDisableTiming));
        v.window_up.push_back(ev2);
    }
    HIP_TRY(ctx, hipMemsetAsync(w.status_dev, 0, n * sizeof(uint32_t), v.up_stream));
    // the packets' headers: on the pool, in (step, slot) order; nobody waits for all of them -- a step's window starts when ITS packets are ready
    {
        std::lock_guard<std::mutex> lk(d->m);
        v.step_pending.assign((size_t)steps, 0);
        for (size_t j = 0; j < n; j++) {
            d->tasks.emplace_back(nullptr, (int)j);
            v.step_pending[(size_t)v.pk[j].ev->t]++;
        }
        d->cv_work.notify_all();
    }
    EntdTotals nt;                       // subsequences, workgroups and header workgroups of the windows enqueued so far
    int next_window = 0;
    // the windows of steps [next_window, upto]: uploads and clears on one stream, the kernels behind them on another
    auto windows_upto = [&](int upto) -> int {
        for (; next_window <= upto && next_window < steps; next_window++) {
            const int t = next_window;
            GopClock wclk;
            gopd_join(d, &v.step_pending[(size_t)t]);
            d->stats[1] += wclk.lap();
            const size_t pa = p0[(size_t)t], pb = p0[(size_t)t + 1], ga = nt.groups;
            const unsigned max_hdr = entd_number(v.pk_host.data(), pa, pb, v.groups_host.data(), nt);
            const size_t gb = nt.groups, ba = byte0[(size_t)t], bb = byte0[(size_t)t + 1];
            if (pb > pa) HIP_TRY(ctx, hipMemcpyAsync(w.pk_dev + pa, v.pk_host.data() + pa, (pb - pa) * sizeof(EdPacket), hipMemcpyHostToDevice, v.up_stream));
            if (gb > ga) HIP_TRY(ctx, hipMemcpyAsync(w.groups_dev + ga, v.groups_host.data() + ga, (gb - ga) * sizeof(uint2), hipMemcpyHostToDevice, v.up_stream));
            if (bb > ba) HIP_TRY(ctx, hipMemcpyAsync(w.bytes_dev + ba, v.bytes_host.data() + ba, bb - ba, hipMemcpyHostToDevice, v.up_stream));
            HIP_TRY(ctx, hipEventRecord(v.window_up[(size_t)t], v.up_stream));
            const hipStream_t es = v.streams[t % v.n_streams];
            HIP_TRY(ctx, hipStreamWaitEvent(es, v.window_up[(size_t)t], 0));
            if (gb > ga) {
                EdBufs b = w.bufs();         // the window's view of the batch-wide arrays: its workgroups, counted from the batch's first
                b.groups += ga; b.packet0 = (uint32_t)pa; b.group0 = (uint32_t)ga;
                entd_launch(es, b, (unsigned)(pb - pa), (unsigned)(gb - ga), max_hdr, v.launches, v.inner);
                const int lrc = launch_check(ctx, "k_entd_*");
                if (lrc) return lrc;
            }
            if (pb > pa) HIP_TRY(ctx, hipMemcpyAsync(w.status_host.data() + pa, w.status_dev + pa, (pb - pa) * sizeof(uint32_t), hipMemcpyDeviceToHost, es));
            HIP_TRY(ctx, hipEventRecord(v.window_done[(size_t)t], es));
            d->stats[3] += wclk.lap();
        }
        return PFV_OK;
    };
    constexpr int kWindowsAhead = 4;     // windows enqueued ahead of the step being decoded (2 .. 15 measured: 1.27-1.38 G whichever, config 4 to HBM)
    if ((rc = windows_upto(kWindowsAhead))) return rc;
    d->stats[3] += clk.lap();

    if ((rc = gopd_continue_run(d, d->gfirst[0] == 2))) return rc;
    if ((rc = gopd_out_room(d, steps))) return rc;
    const int cur0 = hot->cur;
    std::vector<int> key((size_t)G);
    std::vector<uint32_t> combos;
    for (int t = 0; t < steps; t++) {
        const size_t f0 = (size_t)t * S, pa = p0[(size_t)t], pb = p0[(size_t)t + 1];
        if ((rc = windows_upto(t + kWindowsAhead))) return rc;
        clk.lap();
        HIP_TRY(ctx, hipEventSynchronize(v.window_done[(size_t)t]));
        d->stats[5] += clk.lap();
        // what the device stage was not sure about goes through the host parser, which decides
        v.todo.clear();
        for (size_t j = pa; j < pb; j++) {
            GopDevPacket &p = v.pk[j];
            if (p.rc) continue;
            const uint32_t st = w.status_host.data()[j];
            if (st & kEdUnsettled) v.unsettled++;
            else if (st) v.irregular++;
            if (p.host_parse || st) { p.host_parse = true; v.todo.push_back((int)j); }
        }
        for (size_t first = 0; first < v.todo.size(); first += (size_t)kGopDevDense) {
            const int cnt = (int)std::min<size_t>((size_t)kGopDevDense, v.todo.size() - first);
            size_t need = 0;
            for (int j = 0; j < cnt; j++) { v.hp_off[j] = need; need += w.list_room[(size_t)v.todo[first + (size_t)j]]; }
            if (!v.hp_ent.resize(need) || !v.hp_counts.resize((size_t)kGopDevDense * (tb + 1))) return fail(ctx, PFV_ERR_NOMEM, "pinned list staging");
            v.todo_first = (int)first;
            gopd_dev_hostparse_group(d, cnt);
            bool overflowed = false;
            for (int j = 0; j < cnt; j++) {
                const size_t pj = (size_t)v.todo[first + (size_t)j];
                const GopDevPacket &p = v.pk[pj];
                if (p.rc == kSinkFull) overflowed = true;
                if (p.rc) continue;
                if ((rc = upload_lists(ctx, w.lists, p.frame, w.list_room[pj], v.hp_ent.data() + v.hp_off[j], v.hp_n[j], v.hp_counts.data() + (size_t)j * (tb + 1), ctx->stream))) return rc;
                if ((rc = gopd_dev_upload_headers(d, p))) return rc;
            }
            // more values than the packet's bits could hold at three bits each (a one-symbol table: values of one or two bits): once more, with
            // room for every coefficient; its list gets a buffer of its own
            for (int j = 0; overflowed && j < cnt; j++) {
                const size_t pj = (size_t)v.todo[first + (size_t)j];
                GopDevPacket &p = v.pk[pj];
                if (p.rc != kSinkFull) continue;
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if (!v.hp_full.resize(tb * 256)) return fail(ctx, PFV_ERR_NOMEM, "pinned list staging");
                uint8_t q[3];
                p.rc = parse_to_lists(p.ev->payload, p.ev->plen, p.ev->type, tb, d->n_qtables, v.mv_host.data() + p.frame * tb * 2, v.has_host.data() + p.frame * tb, v.hp_full.data(), tb * 256,
                                      v.hp_counts.data() + (size_t)j * (tb + 1), &v.hp_n[j], q);
                if (!p.rc && (rc = upload_lists(ctx, w.lists, p.frame, w.list_room[pj], v.hp_full.data(), v.hp_n[j], v.hp_counts.data() + (size_t)j * (tb + 1), ctx->stream))) return rc;
                if (!p.rc && (rc = gopd_dev_upload_headers(d, p))) return rc;
            }
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // the staging is used again
        }
        if (!v.todo.empty()) d->stats[1] += clk.lap();
        combos.clear();
        for (int k = 0; k < G; k++) key[(size_t)k] = -1;
        for (size_t j = pa; j < pb; j++) {
            GopDevPacket &p = v.pk[j];
            if (!p.rc && !gopd_qidx_ok(hot, p.qidx)) p.rc = PFV_ERR_FORMAT;
            if (p.rc && t == 0 && p.ev->type == 1) {                            // not an independent run after all: the chains change
                gopd_drain_pool(d);                                              // (headers still queued or being read belong to this attempt)
                return 1;
            }
        }
        for (size_t j = pa; j < pb; j++) {
            GopDevPacket &p = v.pk[j];
            const int k = p.ev->slot;
            p.ev->rc = p.rc;
            if (p.rc) {
                p.ev->msg = kGopdBadPayload;
                if ((rc = gopd_hold_slot(d, k))) return rc;
                continue;
            }
            if (p.host_parse) v.packets_host++;
            else v.packets_dev++;
            key[(size_t)k] = gopd_key(combos, p.ev->type, p.qidx);
        }
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, v.window_done[(size_t)t], 0));
        if ((rc = gopd_launch_step(d, t, key, combos, w.mv_dev + f0 * tb * 2, w.has_dev + f0 * tb, w.lists.coefs(f0)))) return rc;
        d->stats[3] += clk.lap();
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    d->stats[4] += clk.lap();
    gopd_close_batch(d, cur0, G - 1, d->glen[(size_t)G - 1]);
    v.batches_dev++;
    return PFV_OK;
}

extern "C" {

PFV_API void pfv_gop_decoder_destroy(pfv_gop_decoder *d)
{
    if (!d) return;
    {
        std::lock_guard<std::mutex> lk(d->m);
        d->quit = true;
        d->cv_work.notify_all();
    }
    for (auto &t : d->workers) t.join();
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    for (GopDecSet &s : d->set)
        if (s.done) (void)hipEventDestroy(s.done);
    if (d->frames_dev) (void)hipFree(d->frames_dev);
    if (d->frames_all_dev) (void)hipFree(d->frames_all_dev);
    for (hipStream_t st : d->dev.streams)
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (d->dev.up_stream) { (void)hipStreamSynchronize(d->dev.up_stream); (void)hipStreamDestroy(d->dev.up_stream); }
    for (hipEvent_t ev : d->dev.window_done) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : d->dev.window_up) (void)hipEventDestroy(ev);
    d->dev.win.destroy();
    pfv_dec_session_destroy(d->hot);
    delete d;
}

// Decoder::new (src/dec.rs:38-134) + the batch shape (see pfv_gop_encoder_create); n_threads: packet parsers besides the calling thread.
PFV_API int pfv_gop_decoder_create(pfv_ctx *ctx, const uint8_t *data, size_t len, int max_gops, int max_gop_frames, int n_threads,
                                   pfv_gop_decoder **out)
{
    if (!ctx || !data || !out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_gop_decoder_create: bad argument");
    *out = nullptr;
    if (max_gops <= 0 || max_gop_frames <= 0 || max_gops > 4096 || max_gop_frames > 4096 || n_threads < 0 || n_threads > 256)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_gop_decoder_create: max_gops and max_gop_frames must be in 1..4096, n_threads in 0..256");
    PfvHeader hd;
    int rc = read_header(ctx, data, len, hd);
    if (rc) return rc;
    const int w = hd.width, h = hd.height, nq = hd.n_qtables;
    if (w > 0 && h > 0 && !(w & 1) && !(h & 1) && (uint64_t)max_gops * (uint64_t)pfv_total_blocks(w, h) * 256u > 0xffffffffull)
        return fail(ctx, PFV_ERR_BAD_ARG, "pfv_gop_decoder_create: max_gops x macroblocks x 256 exceeds the 32-bit coefficient index");
    pfv_dec_session *hot = nullptr;
    if ((rc = pfv_dec_session_create(ctx, w, h, hd.q.data(), nq, max_gops, &hot))) return rc;
    pfv_gop_decoder *d = new pfv_gop_decoder();
    d->ctx = ctx; d->hot = hot; d->data = data; d->len = len;
    d->pos = d->reset_pos = hd.len;
    d->width = w; d->height = h; d->framerate = hd.framerate; d->n_qtables = nq; d->max_gops = max_gops; d->max_len = max_gop_frames;
    d->total_blocks = (size_t)pfv_total_blocks(w, h);
    d->frame_bytes = pfv_frame_bytes(w, h);
    d->cap = d->total_blocks * 256 / 4;                        // per slot: denser than 1 non-zero in 4 -> dense fallback
    const size_t S = (size_t)max_gops, tb = d->total_blocks;
    bool ok = true;
    hipError_t he = hipSuccess;
    for (GopDecSet &s : d->set) {
        ok = s.make(S, d->cap, tb) && ok;
        s.ev.assign(S, nullptr);
        if (ok) { memset(s.mv.data(), 0, S * tb * 2); memset(s.has.data(), 0, S * tb); }
        if (he == hipSuccess) he = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
    }
    // the scatter kernel reads the coefficient lists where the parsers wrote them: that memory must be page-locked (= mapped to the device)
    bool lists_pinned = true;
    for (GopDecSet &s : d->set) lists_pinned = lists_pinned && s.lists_pinned();
    ok = ok && d->frames_host.resize(S * (size_t)max_gop_frames * d->frame_bytes) && d->flags.resize(S * (size_t)max_gop_frames);
    if (ok && he == hipSuccess) he = hipMalloc((void **)&d->frames_dev, S * d->frame_bytes);
    if (!ok) rc = fail(ctx, PFV_ERR_NOMEM, "pfv_gop_decoder_create: host staging");
    else if (!lists_pinned) rc = fail(ctx, PFV_ERR_NOMEM, "pfv_gop_decoder_create: the coefficient-list staging could not be page-locked (locked-memory limit): use a smaller max_gops");
    else if (he != hipSuccess) rc = hip_fail(ctx, he, "pfv_gop_decoder_create");
    if (!rc) rc = dec_staging(hot);
    if (!rc) rc = pfv_dec_set_output_dev(hot, d->frames_dev);
    // the device-entropy path keeps the coefficient arrays of a whole batch in HBM (PFV_OPT_ENTROPY_DECODE)
    GopDecDev &v = d->dev;
    DecWindow &bufs = v.win;
    bool force = false;
    if (entd_take_options(ctx, &force, &v.sub_bits, &v.launches, &v.inner) && !rc && tb > 0) {
        const size_t F = S * (size_t)max_gop_frames;
        // per frame: motion vectors, flags, coded list, counts; the coefficient lists at 4 bytes per 3 payload bits at most (entd_pool_cap)
        const size_t list_guess = std::min(std::min(len, F * (tb * 512 / 8 + 64)) * 8 / 3 + F * 4, F * tb * 256);
        const size_t need = F * tb * (2 + 1 + 4 + 4 + 64) + list_guess * 4;
        size_t free_b = 0, total_b = 0;
        bool fits = hipMemGetInfo(&free_b, &total_b) == hipSuccess && need < free_b / 2;
        if (force) fits = true;
        if (fits) {
            hipError_t e2 = hipSuccess;
            if (getenv("PFV_GOPD_WINDOW_STREAMS")) v.n_streams = std::max(1, std::min((int)GopDecDev::kStreams, atoi(getenv("PFV_GOPD_WINDOW_STREAMS"))));   // experiments
            for (int k = 0; k < v.n_streams && e2 == hipSuccess; k++) e2 = hipStreamCreateWithFlags(&v.streams[k], hipStreamNonBlocking);
            if (e2 == hipSuccess) e2 = hipStreamCreateWithFlags(&v.up_stream, hipStreamNonBlocking);
            if (e2 == hipSuccess && bufs.lists.create(ctx, F, tb, list_guess) != PFV_OK) e2 = hipErrorOutOfMemory;
            if (e2 == hipSuccess) e2 = hipMalloc((void **)&bufs.mv_dev, F * tb * 2);
            if (e2 == hipSuccess) e2 = hipMalloc((void **)&bufs.has_dev, F * tb);
            if (e2 == hipSuccess) e2 = hipMalloc((void **)&bufs.coded_dev, F * tb * 4);
            // a batch's payloads are at most the whole stream: size the staging now, not inside the first batch
            const size_t bytes_guess = std::min(len + F * 32 + 64, F * (tb * 512 / 8 + 64));
            const size_t sub_guess = bytes_guess * 8 / v.sub_bits + F;
            if (e2 == hipSuccess) e2 = hipMalloc((void **)&bufs.bytes_dev, bytes_guess);
            if (e2 == hipSuccess) { bufs.bytes_cap = bytes_guess; e2 = hipMalloc((void **)&bufs.sub_dev, sub_guess * 4 * sizeof(uint32_t)); }
            if (e2 == hipSuccess) { bufs.sub_cap = sub_guess * 4; e2 = hipMalloc((void **)&bufs.groups_dev, (sub_guess / kEdOwn + F) * sizeof(uint2)); }
            if (e2 == hipSuccess) { bufs.groups_cap = sub_guess / kEdOwn + F; e2 = hipMalloc((void **)&bufs.wgsum_dev, bufs.groups_cap * sizeof(unsigned long long)); }
            if (e2 == hipSuccess) { bufs.wgsum_cap = bufs.groups_cap; e2 = hipMalloc((void **)&bufs.pk_dev, F * sizeof(EdPacket)); }
            if (e2 == hipSuccess) e2 = hipMalloc((void **)&bufs.status_dev, F * sizeof(uint32_t));
            if (e2 == hipSuccess) v.pk_cap = F;
            const bool host_ok = e2 == hipSuccess && v.mv_host.resize(F * tb * 2) && v.has_host.resize(F * tb) && v.bytes_host.resize(bytes_guess) &&
                                 v.pk_host.resize(F) && bufs.status_host.resize(F) && v.groups_host.resize(sub_guess / kEdOwn + F);
            if (host_ok) {
                memset(v.mv_host.data(), 0, F * tb * 2);
                memset(v.has_host.data(), 0, F * tb);
                v.frames_cap = F;
                v.on = true;
            } else {
                (void)hipGetLastError();
                bufs.destroy();
                bufs.~DecWindow();
                new (&bufs) DecWindow();        // value-reinitialised (its page-locked members are not assignable): pfv_gop_decoder_destroy meets an empty set
                v.pk_cap = 0;
                for (hipStream_t &st : v.streams)
                    if (st) { (void)hipStreamDestroy(st); st = nullptr; }
                if (v.up_stream) { (void)hipStreamDestroy(v.up_stream); v.up_stream = nullptr; }
                if (force)
                    rc = fail(ctx, PFV_ERR_NOMEM, "pfv_gop_decoder_create: the batch's coefficient arrays do not fit the device (PFV_ENTROPY_DECODE_DEVICE): use a smaller batch");
            }
        }
    }
    if (rc) { pfv_gop_decoder_destroy(d); return rc; }
    for (int t = 0; t < n_threads; t++) d->workers.emplace_back(gopd_worker, d);
    *out = d;
    return PFV_OK;
}
PFV_API int pfv_gop_decoder_width(const pfv_gop_decoder *d) { return d ? d->width : 0; }
PFV_API int pfv_gop_decoder_height(const pfv_gop_decoder *d) { return d ? d->height : 0; }
PFV_API int pfv_gop_decoder_framerate(const pfv_gop_decoder *d) { return d ? d->framerate : 0; }
PFV_API long pfv_gop_decoder_batches(const pfv_gop_decoder *d) { return d ? d->batches : 0; }
/* host seconds so far: out[0] header scan, [1] waiting for packet parsers, [2] waiting for the device before a staging set can be reused,
 * [3] enqueueing (incl. the time since the previous measurement point), [4] waiting for a batch's last frames, [5] waiting for the device's
 * entropy stage; counts: [6] packets whose payload the device read, [7] packets of device-entropy batches the host parser read, of which
 * [8] because the device's read had not settled and [9] because it found the payload irregular; [10] coefficient lists of host-parsed packets that outgrew
 * their place in the list pool and got a buffer of their own (one-symbol tables); returns entries written */
PFV_API int pfv_gop_decoder_stats(const pfv_gop_decoder *d, double *out, int n)
{
    if (!d || !out) return 0;
    const int k = std::min(n, 11);
    const double counts[5] = {(double)d->dev.packets_dev, (double)d->dev.packets_host, (double)d->dev.unsettled, (double)d->dev.irregular, (double)d->dev.win.lists.spilled};
    for (int i = 0; i < k; i++) out[i] = i < 6 ? d->stats[i] : counts[i - 6];
    return k;
}

// on != 0: decoded frames stay in device memory and the callback's y / u / v are DEVICE pointers (valid until the call that starts the next
// batch; ordered on the context's stream, which is idle when the callback runs) -- for consumers on the GPU (the reference README's
// texture-out wish); the download, the whole PCIe cost of decoding, is then not paid.  Only between batches (PFV_ERR_STATE otherwise).
PFV_API int pfv_gop_decoder_set_output_device(pfv_gop_decoder *d, int on)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    if (d->next_event < d->events.size()) return fail(d->ctx, PFV_ERR_STATE, "pfv_gop_decoder_set_output_device: a batch is being delivered");
    d->out_dev = on != 0;
    return PFV_OK;
}

// Decoder::reset (src/dec.rs:148-152).  The framebuffer is NOT rewound (neither is the reference's); unlike the frame-by-frame decoder
// this one has decoded ahead of the frames it delivered, so a stream whose first packet after the reset is a p-frame sees the state of
// the last DECODED frame, not of the last delivered one.  Streams start with an i-frame.
PFV_API int pfv_gop_decoder_reset(pfv_gop_decoder *d)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    d->eof = false;
    d->events.clear(); d->next_event = 0;
    d->pos = d->reset_pos;
    d->cont_valid = false;
    return PFV_OK;
}

// Decoder::advance_frame (src/dec.rs:169-224): 1 = Ok(true), 0 = Ok(false) (EOF), negative = error -- the same sequence of results, frames
// and callbacks as pfv_decoder_advance_frame on the same bytes.  y / u / v stay valid until the call that starts the next batch.
PFV_API int pfv_gop_decoder_advance_frame(pfv_gop_decoder *d, pfv_video_cb onvideo, void *user)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    if (d->eof) return 0;
    if (d->next_event >= d->events.size()) {
        GopClock clk;
        gopd_scan_batch(d);
        d->stats[0] += clk.lap();
        int rc = d->dev.on ? gopd_decode_batch_dev(d) : 1;
        if (rc == 1) {
            if (d->dev.on) d->dev.batches_host++;
            rc = gopd_decode_batch(d);
        }
        if (rc) { gopd_drain_pool(d); d->events.clear(); d->next_event = 0; return rc; }
    }
    GopDecEvent &e = d->events[d->next_event];
    if (e.kind == GopDecEvent::END) { d->pos = e.pos_after; d->eof = true; return 0; }
    if (e.kind == GopDecEvent::ERROR) {   // the next call scans on from where the sequential loop would (src/dec.rs:174-182: the bytes read are gone)
        const int rc = e.rc;
        const char *msg = e.msg;
        d->pos = e.pos_after;
        d->events.clear(); d->next_event = 0;
        return fail(d->ctx, rc, msg);
    }
    d->next_event++;
    d->pos = e.pos_after;
    if (e.kind == GopDecEvent::DROP) return 1;
    if (e.rc) return fail(d->ctx, e.rc, e.msg);
    if (onvideo) {
        const uint8_t *f = (d->out_dev ? d->frames_all_dev : d->frames_host.data()) + ((size_t)e.t * (size_t)d->max_gops + (size_t)e.slot) * d->frame_bytes;
        const size_t ny = (size_t)d->width * d->height, nc = (size_t)(d->width / 2) * (d->height / 2);
        onvideo(user, f, f + ny, f + ny + nc, d->width, d->height);
    }
    return 1;
}

// Decoder::advance_delta (src/dec.rs:154-167)
PFV_API int pfv_gop_decoder_advance_delta(pfv_gop_decoder *d, double delta, pfv_video_cb onvideo, void *user)
{
    if (!d) return fail(nullptr, PFV_ERR_BAD_ARG, "null decoder");
    d->delta_accum += delta;
    const double delta_per_frame = 1.0 / (double)d->framerate;
    while (d->delta_accum >= delta_per_frame) {
        int rc = pfv_gop_decoder_advance_frame(d, onvideo, user);
        if (rc <= 0) return rc;
        d->delta_accum -= delta_per_frame;
    }
    return 1;
}

}  // extern "C"
