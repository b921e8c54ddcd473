// pfv_stream_objects.hip -- stream-level objects, first half: pfv_encoder (enc::Encoder<W>), the staging types the three decoder objects share, the host half of the decoders' device entropy stage.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.
// ================================================================== stream-level session objects
// enc::Encoder<W> (src/enc.rs:12-188) with W = an in-memory byte vector (the reference's tests use
// Cursor<Vec<u8>>, src/lib.rs:319-321), dec::Decoder<R> (src/dec.rs:15-224) with R = a caller-owned byte slice.
// Page-locked host staging (hipHostMalloc): PCIe copies from / to these run at link rate without the runtime's
// bounce through its own pinned chunks; where page-locking is refused the buffer is ordinary memory.
template <class T>
struct PinnedBuf {
    T *p = nullptr;
    size_t n = 0;
    bool pinned = false;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    void release()
    {
        if (p && pinned) (void)hipHostFree(p);
        else if (p) free(p);
        p = nullptr; n = 0;
    }
    bool resize(size_t count)
    {
        if (count <= n) return true;
        release();
        if (hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault) == hipSuccess) {
            pinned = true;
        } else {   // locked-memory limits: pageable memory still works, the copies just bounce through the runtime
            (void)hipGetLastError();
            p = (T *)malloc(count * sizeof(T));
            pinned = false;
            if (!p) return false;
        }
        n = count;
        return true;
    }
    T *data() { return p; }
    size_t size() const { return n; }
    void swap(PinnedBuf &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(pinned, o.pinned); }
};
// Room for `need` elements in a grow-only device buffer: a new one is made need / grow_div larger than asked.  `busy`: the stream to wait for
// before the old buffer is freed; nullptr when the caller knows that nothing on the device uses it any more.
template <class T>
static int dev_room(pfv_ctx *ctx, T **p, size_t *cap, size_t need, size_t grow_div, const hipStream_t *busy = nullptr)
{
    if (need <= *cap) return PFV_OK;
    if (*p) {
        if (busy) HIP_TRY(ctx, hipStreamSynchronize(*busy));
        (void)hipFree(*p); *p = nullptr; *cap = 0;
    }
    need += need / grow_div;
    HIP_TRY(ctx, hipMalloc((void **)p, need * sizeof(T)));
    *cap = need;
    return PFV_OK;
}

struct pfv_encoder {
    pfv_ctx *ctx = nullptr;
    pfv_enc_session *hot = nullptr;
    int width = 0, height = 0, framerate = 0, total_blocks = 0;
    bool finished = false;
    bool device_entropy = true;            // payloads built by the k_ent_* kernels instead of serialize_*frame on the host
    const uint8_t *plane[3] = {nullptr, nullptr, nullptr};   // device path: the caller's planes of the frame being encoded
    bool poisoned = false;                 // a frame failed after prev_frame had moved on: the next frame must be an i-frame
    std::vector<uint8_t> out;              // the writer: bytes produced and not yet handed over (pfv_encoder_drain)
    std::vector<uint8_t> drained;          // what the last pfv_encoder_drain handed over
    PinnedBuf<uint8_t> frame;              // packed Y|U|V staging
    PinnedBuf<int16_t> coef;               // host entropy path only
    PinnedBuf<int8_t> mv;
    PinnedBuf<uint8_t> has;
    PinnedBuf<uint8_t> payload;            // device entropy path: packet payload landing zone
    // frame reports (pfv_encoder_set_frame_report): the plane sums land in `sums` with the frame's other downloads
    bool report_on = false;
    int report_state = 0;                  // 0: no encode_* call yet, 1: `report` describes the last one, -1: the last one failed
    pfv_frame_report report{};
    PinnedBuf<uint64_t> sums;              // [3]
    // frame SSIM (pfv_encoder_set_frame_ssim): a switch of its own, the same life cycle
    bool ssim_on = false;
    int ssim_state = 0;                    // as report_state
    pfv_frame_ssim ssim{};
    PinnedBuf<int64_t> ssim_sums;          // [3]
    // quality ladder (pfv_encoder_create_ladder): the current rung is the session's; rate control (pfv_encoder_set_rate)
    int last_rung = -1;                    // rung of the last frame written (-1: none yet)
    uint32_t budget_p = 0;                 // p-frame payload bytes; 0: off
    uint32_t budget_i = 0;                 // i-frame payload bytes (pfv_encoder_set_iframe_budget); 0: off
    double floor_i = 0.0;                  // i-frame PSNR-YUV floor in dB (pfv_encoder_set_iframe_quality_floor); 0: off
    double floor_p = 0.0;                  // p-frame PSNR-YUV floor in dB (pfv_encoder_set_pframe_quality_floor); 0: off
    double sfloor_i = 0.0;                 // i-frame floor on the frame's mean SSIM (pfv_encoder_set_iframe_ssim_floor); 0: off
    double sfloor_p = 0.0;                 // p-frame floor on the frame's mean SSIM (pfv_encoder_set_pframe_ssim_floor); 0: off
    // p-frame size probe (pfv_encoder_set_pframe_probe): the hard p-frame budget; automatic frame types (pfv_encoder_encode_frame)
    bool pprobe_on = false;
    int gop_max = 0;                       // pfv_encoder_set_gop: an i-frame is forced once this many frames have followed the last one; 0: never
    uint64_t n_written = 0;                // frames written, drop frames included
    int since_iframe = 0;                  // frames written behind the last i-frame, drop frames included
    // RGB picture input (pfv_encoder_set_input_rgb): `y` of every call is one tight picture, u and v are NULL
    bool rgb_on = false;
    int rgb_format = 0, rgb_chroma = 0;    // PFV_PIX_*, PFV_CHROMA_*
    uint8_t *rgb_scratch = nullptr;        // device: where the picture waits for k_ingest_rgb; holds any format; made by the set call
    size_t rgb_scratch_cap = 0;
    // resized input (pfv_encoder_set_input_size): the (y, u, v) -- or the picture -- of every call have the size src_w x src_h
    pfv_scaler *scaler = nullptr;          // src_w x src_h -> width x height; owned
    int src_w = 0, src_h = 0;
    uint8_t *scale_src = nullptr;          // device: the packed frame of the source size that waits for k_scale; made by the set call
    // denoising pre-filter (pfv_encoder_set_denoise): the last input stage, between the stages above and the session's frame staging
    bool dn_on = false;
    pfv_denoiser *dn = nullptr;            // one stream of width x height; owned; made by the set call
    uint8_t *dn_src = nullptr;             // device: the packed frame that waits for k_denoise; made by the set call
    bool dn_commit = false;                // the entry point that is running commits (encode_*) or does not (probe_*)
    bool dn_staged = false;                // ... and its filtered (or measured) frame lies in the staging already: an upload is not repeated
    // scene-cut detection (pfv_encoder_set_scene_cut): every entry point that stages a frame measures it once, behind the input stages
    bool sc_on = false;
    pfv_scene_detector *sc = nullptr;      // one stream of width x height; owned; made by the set call
    pfv_scene_stats *sc_dev = nullptr;     // device: where k_scene_sum writes; made by the set call
    PinnedBuf<pfv_scene_stats> sc_host;    // [1]: arrives with the entry point's next synchronisation
    bool sc_measured = false;              // a frame has been measured since the switch went on
    uint32_t sc_threshold = PFV_SCENE_THRESHOLD_DEFAULT;
    int sc_min_interval = 0;
};

// One step of Decoder::advance_frame's packet loop (src/dec.rs:169-224), found by the header scanner.  FRAME events are
// parsed (bits -> coefficients / block headers, dec.rs:226-296, 328-417) ahead of their turn by worker threads: packets
// are independent bit streams, only the device decode behind them is sequential.
// ------------------------------------------------------------------ the decoders' entropy stage on the device: host half
// What the host reads of a packet for the k_entd_* kernels (pfv_entdec_kernels.hip): its first 19 bytes -- the table (-> the tree's codes) and
// the q indices.  A p-frame's block headers are read on the device since round 5 (k_hdr_*: motion vectors, has_coeff, the first bit of the run
// streams), the list of coded macroblocks is made there from the has_coeff bytes (k_entd_coded).
// The payload is copied to `bytes_dst` (page-locked staging, >= plen + 16 bytes).  The caller has set k.byte_off / k.frame_off.
// A packet the host has to read (rc or host_parse) is left with n_sub = hdr_wgs = 0: it gets no workgroup in its window (entd_number).
// header workgroups (k_hdr_*) of a p-frame packet: 2 048 bits each, as many as its headers can take (16 bits per macroblock) or its payload has
static inline uint32_t entd_hdr_wgs(size_t tb, size_t plen)
{
    const size_t bits = plen * 8 > kHdrBit0 ? plen * 8 - kHdrBit0 : 0;
    return (uint32_t)((std::min(bits, tb * 16) + kHdrWgBits - 1) / kHdrWgBits);
}
struct EntdPrep {
    int rc = 0;                  // a status the host parser would have returned before it read any run (header, q index, truncated block headers)
    bool host_parse = false;     // the host parser has to read this packet (degenerate code table, 512 MiB or more, no bits behind the headers)
    uint8_t qidx[3] = {0, 0, 0};
};
static EntdPrep entd_prepare(const uint8_t *payload, uint32_t plen, int type, size_t tb, int n_qtables, uint32_t sub_bits, EdPacket &k, uint8_t *bytes_dst)
{
    EntdPrep p;
    k.total_bits = k.bit0 = k.total_coefs = k.n_sub = k.sub_first = k.grp_first = k.list_cap = 0;
    k.org = k.first_sub = k.hdr_first = k.hdr_wgs = 0;
    k.sub_bits = sub_bits;
    k.pframe = type == 2 ? 1u : 0u;
    k.total_blocks = (uint32_t)tb;
    memset(k.code_val, 0, sizeof k.code_val);
    memset(k.code_len, 0, sizeof k.code_len);
    BitSource r(payload, plen);
    PacketHead h;
    p.rc = parse_head(r, h, n_qtables);
    if (p.rc) return p;
    memcpy(p.qidx, h.qidx, 3);
    int n_syms = 0;
    for (uint8_t t : h.table) n_syms += t != 0;
    const uint64_t bits = (uint64_t)plen * 8, bit0 = r.position();      // behind the table and the q indices: bit 152
    // zero-length codes / no bits left / 64 MiB and more: a run costs two bits or more and covers at most 16 coefficients, so below 2^29 bits
    // the kernels' counters (coefficients and values per packet, 32 bits each, summed side by side in one 64-bit word) cannot overflow
    if (n_syms < 2 || bits >= (1ull << 29) || bit0 >= bits) { p.host_parse = true; return p; }
    HuffmanTree tree(h.table);
    for (int s = 0; s < 16; s++) {
        k.code_val[s] = (uint16_t)tree.code((uint8_t)s).val;
        k.code_len[s] = (uint8_t)tree.code((uint8_t)s).len;
    }
    k.total_bits = (uint32_t)bits;
    k.bit0 = k.org = (uint32_t)bit0;
    k.n_sub = (uint32_t)((bits - bit0 + sub_bits - 1) / sub_bits);
    if (type == 2) {
        // the block headers (src/dec.rs:351-372) are read on the device (k_hdr_*): where the run streams start, how many macroblocks are coded
        // and what the list can need is written into the descriptor there; the subsequences are counted from bit 152
        k.hdr_wgs = entd_hdr_wgs(tb, plen);
    } else {
        k.total_coefs = (uint32_t)(tb * 256);
        k.list_cap = (uint32_t)std::min<uint64_t>(tb * 256, (bits - bit0) / 3 + 1);   // <= entd_pool_cap(tb, plen): the room the caller set aside
    }
    memcpy(bytes_dst, payload, plen);
    memset(bytes_dst + plen, 0, 16);
    return p;
}
// Entries a packet's coefficient list can need, known before any of it is read: a value costs three bits or more (two tree codes of a bit or
// more -- tables of fewer than two symbols go to the host parser -- and coeff_size >= 1 value bits), and there are no more values than
// coefficients.  Rounded up to whole 16-byte lines so that the lists of a pool start aligned.
static inline size_t entd_pool_cap(size_t tb, size_t plen) { return (std::min(tb * 256, plen * 8 / 3 + 1) + 3) & ~(size_t)3; }

// Device side of the coefficient lists of `frames` frames (pfv_device.h: CoefLists): a pool of entries the frames' lists are cut from, the
// table of list pointers the decode kernels index by slot, the frames' counts.  A list that does not fit its place in the pool -- only a
// packet the HOST parser read can need more than entd_pool_cap (a one-symbol table: values of one or two bits) -- gets a buffer of its own
// for the life of the batch (spill).
struct ListPool {
    uint32_t *ent = nullptr; size_t ent_cap = 0;       // entries
    uint32_t **ptr_dev = nullptr;                      // [frames]
    uint32_t *counts_dev = nullptr;                    // [frames][tb + 1]
    size_t frames = 0, tb = 0;
    PinnedBuf<uint32_t *> ptr_host;
    std::vector<uint32_t *> spill;
    long spilled = 0;                                  // lists that got a buffer of their own so far
    int create(pfv_ctx *ctx, size_t n_frames, size_t total_blocks, size_t entries)
    {
        frames = n_frames; tb = total_blocks;
        HIP_TRY(ctx, hipMalloc((void **)&ptr_dev, n_frames * sizeof(uint32_t *)));
        HIP_TRY(ctx, hipMalloc((void **)&counts_dev, n_frames * (total_blocks + 1) * sizeof(uint32_t)));
        if (entries) { HIP_TRY(ctx, hipMalloc((void **)&ent, entries * sizeof(uint32_t))); ent_cap = entries; }
        if (!ptr_host.resize(n_frames)) return fail(ctx, PFV_ERR_NOMEM, "pinned list-pointer staging");
        for (size_t f = 0; f < n_frames; f++) ptr_host.data()[f] = nullptr;
        return PFV_OK;
    }
    // room for `entries` in the pool; the caller has made sure nothing on the device still uses it
    int room(pfv_ctx *ctx, size_t entries)
    {
        if (entries <= ent_cap) return PFV_OK;
        if (ent) { (void)hipFree(ent); ent = nullptr; ent_cap = 0; }
        entries += entries / 4;
        HIP_TRY(ctx, hipMalloc((void **)&ent, entries * sizeof(uint32_t)));
        ent_cap = entries;
        return PFV_OK;
    }
    void drop_spill()
    {
        for (uint32_t *p : spill) (void)hipFree(p);
        spill.clear();
    }
    void destroy()
    {
        drop_spill();
        for (void *p : {(void *)ent, (void *)ptr_dev, (void *)counts_dev})
            if (p) (void)hipFree(p);
        ent = nullptr; ptr_dev = nullptr; counts_dev = nullptr; ent_cap = 0;
    }
    DecCoefs coefs(size_t first_frame = 0) const { return DecCoefs(ptr_dev + first_frame, counts_dev + first_frame * (tb + 1)); }
};

// A packet through the HOST parser into list form, for a decoder whose coefficients travel as lists: entries and counts into page-locked
// staging (`ent` with room for `cap` entries, `counts` [tb + 1]).  kSinkFull: more than `cap` entries (parse again with room for tb x 256).
static int parse_to_lists(const uint8_t *payload, size_t plen, int type, size_t tb, int n_qtables, int8_t *mv, uint8_t *has, uint32_t *ent, size_t cap, uint32_t *counts,
                          size_t *n_out, uint8_t qidx[3])
{
    ListSink sink{ent, cap, counts, tb};
    const int rc = parse_frame_to(type, payload, plen, (int)tb, n_qtables, mv, has, sink, qidx);
    sink.finish();
    *n_out = sink.n;
    return rc;
}
// ... and onto the device, in frame `f`'s place of the pool (or a buffer of its own when it is longer than the place: `place_cap` entries),
// on `stream`; the staging is free again when the stream has passed this point
static int upload_lists(pfv_ctx *ctx, ListPool &lp, size_t f, size_t place_cap, const uint32_t *ent, size_t n, const uint32_t *counts, hipStream_t stream)
{
    uint32_t *dst = lp.ptr_host.data()[f];
    if (n > place_cap || !dst) {
        HIP_TRY(ctx, hipMalloc((void **)&dst, std::max<size_t>(n, 1) * sizeof(uint32_t)));
        lp.spill.push_back(dst);
        lp.spilled++;
        lp.ptr_host.data()[f] = dst;
        HIP_TRY(ctx, hipMemcpyAsync(lp.ptr_dev + f, lp.ptr_host.data() + f, sizeof(uint32_t *), hipMemcpyHostToDevice, stream));
    }
    if (n) HIP_TRY(ctx, hipMemcpyAsync(dst, ent, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(lp.counts_dev + f * (lp.tb + 1), counts, (lp.tb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    return PFV_OK;
}

// the launches of one window: np packets from b.packet0 on, ng workgroups from b.group0 on (b.groups already points at the first of them)
static void entd_launch(hipStream_t stream, const EdBufs &b, unsigned np, unsigned ng, unsigned max_hdr_wgs, int launches, int inner)
{
    if (max_hdr_wgs) {   // the p-frames' block headers first: they complete the packet descriptors the kernels below read
        hipLaunchKernelGGL(k_hdr_map, dim3(max_hdr_wgs, np), dim3(kEdThreads), 0, stream, b);
        hipLaunchKernelGGL(k_hdr_scan, dim3(np), dim3(kEdThreads), 0, stream, b);
        hipLaunchKernelGGL(k_hdr_emit, dim3(max_hdr_wgs, np), dim3(kEdThreads), 0, stream, b);
    }
    hipLaunchKernelGGL(k_entd_coded, dim3(np), dim3(kEdThreads), 0, stream, b);
    hipLaunchKernelGGL(k_entd_sync, dim3(ng), dim3(kEdThreads), 0, stream, b, inner);                      // every subsequence, settled inside the workgroups
    for (int round = 1; round < launches; round++)                                                           // the seams between them (a second pass finds nothing, as a rule)
        hipLaunchKernelGGL(k_entd_fix, dim3((ng + kEdFixThreads - 1) / kEdFixThreads), dim3(kEdFixThreads), 0, stream, b, (uint32_t)ng);
    hipLaunchKernelGGL(k_entd_verify, dim3(ng), dim3(kEdThreads), 0, stream, b);
    hipLaunchKernelGGL(k_entd_prefix, dim3(np), dim3(kEdThreads), 0, stream, b);
    hipLaunchKernelGGL(k_entd_emit, dim3(ng), dim3(kEdThreads), 0, stream, b);
}

// Numbers the packets [pa, pb) of a window -- their first subsequence, workgroup and header workgroup among all of the descriptor array's, counted
// on in `n` -- and lists their workgroups (packet, which kEdOwn subsequences of it) in `groups` from n.groups on.  Returns the most header
// workgroups any of them has.
struct EntdTotals { size_t sub = 0, groups = 0, hdr = 0; };
static unsigned entd_number(EdPacket *pk, size_t pa, size_t pb, uint2 *groups, EntdTotals &n)
{
    unsigned max_hdr = 0;
    for (size_t j = pa; j < pb; j++) {
        EdPacket &k = pk[j];
        k.sub_first = (uint32_t)n.sub;
        k.grp_first = (uint32_t)n.groups;
        k.hdr_first = (uint32_t)n.hdr;
        n.sub += k.n_sub;
        n.hdr += k.hdr_wgs;
        max_hdr = std::max(max_hdr, (unsigned)k.hdr_wgs);
        for (uint32_t blk = 0; blk * (uint32_t)kEdOwn < k.n_sub; blk++) groups[n.groups++] = make_uint2((unsigned)j, blk);
    }
    return max_hdr;
}

struct DecEvent {
    enum Kind { FRAME, DROP, END, ERROR } kind = END;
    enum State { FREE, QUEUED, RUNNING, DONE } state = FREE;
    int rc = 0;                          // ERROR: the status to return; FRAME: parse result
    const char *msg = "";
    uint8_t type = 0;                    // FRAME: 1 = i-frame, 2 = p-frame
    size_t pos_after = 0;                // stream position once this event has been consumed
    const uint8_t *payload = nullptr;
    uint32_t plen = 0;
    uint8_t qidx[3] = {0, 0, 0};
    PinnedBuf<int16_t> coef;             // dense form: only when the sparse list overflowed
    PinnedBuf<int8_t> mv;
    PinnedBuf<uint8_t> has;
    PinnedBuf<uint32_t> idx;             // sparse form: non-zero coefficients as (flat index, value)
    PinnedBuf<int16_t> val;
    size_t n_sparse = 0;
    bool dense = false;
    // device-entropy form (PFV_OPT_ENTROPY_DECODE): what entd_prepare left for the k_entd_* kernels instead of a parsed packet
    bool dev_form = false, host_parse = false;
    PinnedBuf<uint8_t> bytes;            // the payload (+ 16)
    PinnedBuf<EdPacket> pk;              // 1
    PinnedBuf<uint2> groups;             // workgroups of the packet (entd_window_enqueue)
};

// switches, shape and counters of the device entropy stage in pfv_decoder / pfv_batch_decoder (the buffers: DecWindow)
struct DecEntd {
    std::atomic<bool> on{false};         // read by the parser threads; cleared by the caller's thread when the window sets cannot be made (AUTO: the host parser takes over)
    bool force = false;                  // force: every packet (PFV_ENTROPY_DECODE_DEVICE); otherwise payloads of kDecEntdMinBytes and more
    bool ready = false;                  // the window stream and the window sets exist: made by the first packet / step that takes the device form
    //                                      (a decoder of small packets never needs them), entd_windows_make
    uint32_t sub_bits = kEdSubBits;
    int launches = 3, inner = kEdInner;
    long packets_dev = 0, packets_host = 0;
};
constexpr uint32_t kDecEntdMinBytes = 64 * 1024;   // below this the launches cost more than the host parser needs for the packet
// the stage's options as the context has them now (PFV_OPT_ENTROPY_DECODE, PFV_OPT_ENTDEC_*); false: the host parser reads every packet
static bool entd_take_options(const pfv_ctx *ctx, bool *force, uint32_t *sub_bits, int *launches, int *inner)
{
    *force = ctx->opt_entropy_decode == PFV_ENTROPY_DECODE_DEVICE;
    *sub_bits = (uint32_t)ctx->opt_entdec_lane_bits; *launches = ctx->opt_entdec_launches; *inner = ctx->opt_entdec_inner;
    return ctx->opt_entropy_decode != PFV_ENTROPY_DECODE_HOST;
}

// device side of one packet's window in pfv_decoder.  Two alternate: the window of the NEXT packet (uploads, k_entd_*, status) runs on a
// second stream under the decode launch and the frame download of the current one.
struct DecWindow {
    uint8_t *bytes_dev = nullptr; size_t bytes_cap = 0;
    uint2 *groups_dev = nullptr; size_t groups_cap = 0;
    uint32_t *sub_dev = nullptr; size_t sub_cap = 0;
    EdPacket *pk_dev = nullptr;
    uint32_t *status_dev = nullptr, *coded_dev = nullptr;
    unsigned long long *wgsum_dev = nullptr; size_t wgsum_cap = 0;
    uint32_t *hdr_maps_dev = nullptr; size_t hdr_maps_cap = 0;      // k_hdr_*: [header workgroup][8]
    uint4 *hdr_start_dev = nullptr; size_t hdr_start_cap = 0;       // [header workgroup]
    ListPool lists;                      // the window's coefficients: one list per packet (pfv_device.h: CoefLists)
    std::vector<size_t> list_room;       // per packet: the size of its list's place in the pool
    int8_t *mv_dev = nullptr;
    uint8_t *has_dev = nullptr;
    PinnedBuf<uint32_t> status_host;
    hipEvent_t done = nullptr;
    const void *owner = nullptr;         // an identity only: the packet (pfv_decoder) or staging set (pfv_batch_decoder) whose window is enqueued on this set
    EdBufs bufs() const                  // the kernels' view of the set: packets and workgroups count from 0
    {
        const size_t ts = sub_cap / 4;
        return EdBufs{bytes_dev, pk_dev, groups_dev, sub_dev, sub_dev + ts, sub_dev + 2 * ts, wgsum_dev, coded_dev, lists.ptr_dev, lists.counts_dev, status_dev, 0u, 0u,
                      hdr_maps_dev, hdr_start_dev, mv_dev, has_dev};
    }
    void destroy()
    {
        for (void *p : {(void *)bytes_dev, (void *)pk_dev, (void *)status_dev, (void *)coded_dev, (void *)groups_dev, (void *)sub_dev, (void *)wgsum_dev, (void *)mv_dev, (void *)has_dev,
                        (void *)hdr_maps_dev, (void *)hdr_start_dev})
            if (p) (void)hipFree(p);
        lists.destroy();
        if (done) (void)hipEventDestroy(done);
    }
};

// The window stream and the fixed-size part of every window set, for S packets per window: on the caller's thread, when the first packet (step)
// takes the device form.
template <size_t N>
static int entd_windows_make(pfv_ctx *ctx, DecEntd &v, DecWindow (&win)[N], hipStream_t *stream, size_t S, size_t tb)
{
    if (v.ready) return PFV_OK;
    hipError_t he = *stream ? hipSuccess : hipStreamCreateWithFlags(stream, hipStreamNonBlocking);
    bool host_ok = true;
    for (DecWindow &w : win) {
        if (he == hipSuccess && !w.pk_dev) he = hipMalloc((void **)&w.pk_dev, S * sizeof(EdPacket));
        if (he == hipSuccess && !w.status_dev) he = hipMalloc((void **)&w.status_dev, S * sizeof(uint32_t));
        if (he == hipSuccess && !w.coded_dev) he = hipMalloc((void **)&w.coded_dev, S * tb * sizeof(uint32_t));
        if (he == hipSuccess && !w.lists.ptr_dev && w.lists.create(ctx, S, tb, 0) != PFV_OK) he = hipErrorOutOfMemory;
        if (he == hipSuccess && !w.mv_dev) he = hipMalloc((void **)&w.mv_dev, S * tb * 2);
        if (he == hipSuccess && !w.has_dev) he = hipMalloc((void **)&w.has_dev, S * tb);
        if (he == hipSuccess && !w.done) he = hipEventCreateWithFlags(&w.done, hipEventDisableTiming);
        host_ok = host_ok && w.status_host.resize(S);
    }
    if (he != hipSuccess) return hip_fail(ctx, he, "device entropy stage: window sets");
    if (!host_ok) return fail(ctx, PFV_ERR_NOMEM, "device entropy stage: pinned status words");
    v.ready = true;
    return PFV_OK;
}
// host staging of one packet the host parser reads into list form (a decoder whose coefficients travel as lists)
struct ListStage {
    PinnedBuf<uint32_t> ent, counts;
    size_t n = 0;
    // kSinkFull cannot come back: a list of the place's size is tried first, then one with room for every coefficient
    int parse(const uint8_t *payload, size_t plen, int type, size_t tb, int n_qtables, int8_t *mv, uint8_t *has, size_t place_cap, uint8_t qidx[3])
    {
        if (!ent.resize(std::max<size_t>(place_cap, 4)) || !counts.resize(tb + 1)) return PFV_ERR_NOMEM;
        int rc = parse_to_lists(payload, plen, type, tb, n_qtables, mv, has, ent.data(), place_cap, counts.data(), &n, qidx);
        if (rc != kSinkFull) return rc;
        if (!ent.resize(tb * 256)) return PFV_ERR_NOMEM;
        return parse_to_lists(payload, plen, type, tb, n_qtables, mv, has, ent.data(), tb * 256, counts.data(), &n, qidx);
    }
};
// host staging of one frame step of S slots whose packets the HOST parser reads (pfv_batch_decoder, pfv_gop_decoder): per slot an (index,
// value) list of `cap` entries with flat indices into [slot][macroblock][256], the block headers, the parse status and the q indices.  One
// segmented scatter kernel reads the lists where the parsers wrote them (page-locked memory).
struct StepStage {
    PinnedBuf<uint32_t> idx;
    PinnedBuf<int16_t> val;
    PinnedBuf<uint32_t> counts;
    PinnedBuf<int8_t> mv;
    PinnedBuf<uint8_t> has;
    std::vector<int> rc;               // per slot: 0, kSinkFull (the list overflowed: dense fallback), PFV_ERR_*
    std::vector<uint8_t> qidx;         // per slot x 3
    bool make(size_t S, size_t cap, size_t tb)
    {
        rc.assign(S, 0); qidx.assign(S * 3, 0);
        return idx.resize(S * cap) && val.resize(S * cap) && counts.resize(S) && mv.resize(S * tb * 2) && has.resize(S * tb);
    }
    bool lists_pinned() const { return idx.pinned && val.pinned && counts.pinned; }   // the scatter kernel can read them
    // slot k's packet.  Only a packet that parsed leaves a count: a list that overflowed or broke off is never scattered -- pfv_gop_decoder
    // does not launch such a slot (or uploads its dense form over it), pfv_batch_decoder scatters no step that has one.
    void parse(int k, int type, const uint8_t *payload, size_t len, size_t tb, int n_qtables, size_t cap)
    {
        SparseSink sink{idx.data() + (size_t)k * cap, val.data() + (size_t)k * cap, cap};
        sink.offset = (size_t)k * tb * 256;
        rc[(size_t)k] = parse_frame_to(type, payload, len, (int)tb, n_qtables, mv.data() + (size_t)k * tb * 2, has.data() + (size_t)k * tb, sink, &qidx[(size_t)k * 3]);
        counts.data()[k] = rc[(size_t)k] == 0 ? (uint32_t)sink.n : 0u;
    }
    // the lists of slots [0, S) into the session's cleared coefficient staging, on the context's stream
    int scatter(pfv_ctx *ctx, pfv_dec_session *hot, size_t S, size_t tb, size_t cap)
    {
        const size_t total = tb * S * 256;
        HIP_TRY(ctx, hipMemsetAsync(hot->st_coef, 0, total * 2, ctx->stream));
        hipLaunchKernelGGL(k_scatter_coef_seg, dim3(64, (unsigned)S), dim3(kThreads), 0, ctx->stream, idx.data(), val.data(), counts.data(), (uint32_t)cap, (uint32_t)total,
                           hot->st_coef);
        return launch_check(ctx, "k_scatter_coef_seg");
    }
};

// One window of the stage on set w, all on `st`: the S packets entd_prepare left in `pk` (payloads of `plen` bytes copied to `bytes` at their
// byte_off, `bytes_total` in all) are numbered, go up with their workgroup list, k_hdr_* / k_entd_* read them into the set's lists, the
// statuses come down and w.done is recorded.  S and the macroblock count are the set's (entd_windows_make).  The set is idle: its last window
// was consumed and decoded.
static int entd_window_enqueue(pfv_ctx *ctx, const DecEntd &v, DecWindow &w, hipStream_t st, EdPacket *pk, const uint8_t *bytes, size_t bytes_total, const size_t *plen,
                               PinnedBuf<uint2> &groups, const void *owner)
{
    const size_t S = w.lists.frames, tb = w.lists.tb;
    size_t n_groups = 0;
    for (size_t k = 0; k < S; k++) n_groups += (pk[k].n_sub + kEdOwn - 1) / kEdOwn;
    if (!groups.resize(n_groups + 1)) return fail(ctx, PFV_ERR_NOMEM, "pinned staging");
    EntdTotals n;
    const unsigned max_hdr = entd_number(pk, 0, S, groups.data(), n);
    if (n.sub >= 0xffffffffull) return fail(ctx, PFV_ERR_NOMEM, "device entropy stage: payloads too large for one window");
    int rc;
    if ((rc = dev_room(ctx, &w.bytes_dev, &w.bytes_cap, bytes_total + 64, 2))) return rc;
    if ((rc = dev_room(ctx, &w.groups_dev, &w.groups_cap, n_groups + 1, 2))) return rc;
    if ((rc = dev_room(ctx, &w.sub_dev, &w.sub_cap, (n.sub + 1) * 4, 2))) return rc;
    if ((rc = dev_room(ctx, &w.wgsum_dev, &w.wgsum_cap, n_groups + 1, 2))) return rc;
    if ((rc = dev_room(ctx, &w.hdr_maps_dev, &w.hdr_maps_cap, (n.hdr + 1) * 8, 2))) return rc;
    if ((rc = dev_room(ctx, &w.hdr_start_dev, &w.hdr_start_cap, n.hdr + 1, 2))) return rc;
    // every packet's list: its place in the window's pool from the packet's size
    size_t total = 0;
    w.list_room.assign(S, 0);
    for (size_t k = 0; k < S; k++) { w.list_room[k] = entd_pool_cap(tb, plen[k]); total += w.list_room[k]; }
    w.lists.drop_spill();
    if ((rc = w.lists.room(ctx, total))) return rc;
    total = 0;
    for (size_t k = 0; k < S; k++) { w.lists.ptr_host.data()[k] = w.lists.ent + total; total += w.list_room[k]; }
    HIP_TRY(ctx, hipMemcpyAsync(w.lists.ptr_dev, w.lists.ptr_host.data(), S * sizeof(uint32_t *), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(w.bytes_dev, bytes, bytes_total, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(w.pk_dev, pk, S * sizeof(EdPacket), hipMemcpyHostToDevice, st));
    if (n_groups) HIP_TRY(ctx, hipMemcpyAsync(w.groups_dev, groups.data(), n_groups * sizeof(uint2), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(w.status_dev, 0, S * sizeof(uint32_t), st));
    if (n_groups) {
        entd_launch(st, w.bufs(), (unsigned)S, (unsigned)n_groups, max_hdr, v.launches, v.inner);
        if ((rc = launch_check(ctx, "k_entd_*"))) return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(w.status_host.data(), w.status_dev, S * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipEventRecord(w.done, st));
    w.owner = owner;
    return PFV_OK;
}
// Packet k of window w is for the host parser (the device stage was not certain about it, or could not take it): the parser reads it into `hp`
// and decides; its list goes up into the packet's place on `stream`, a p-frame's block headers with it (the device's read of them is not what
// is decoded).  `hp` is free again when `stream` has passed this point.  Returns the parser's status, or that of a failed upload.
static int entd_host_parse(pfv_ctx *ctx, ListStage &hp, DecWindow &w, size_t k, const uint8_t *payload, size_t plen, int type, int n_qtables, int8_t *mv, uint8_t *has, uint8_t qidx[3],
                           hipStream_t stream)
{
    const size_t tb = w.lists.tb;
    const int prc = hp.parse(payload, plen, type, tb, n_qtables, mv, has, w.list_room[k], qidx);
    if (prc) return fail(ctx, prc, prc == PFV_ERR_NOMEM ? "pinned list staging" : "malformed packet payload");
    const int rc = upload_lists(ctx, w.lists, k, w.list_room[k], hp.ent.data(), hp.n, hp.counts.data(), stream);
    if (rc || type != 2) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(w.mv_dev + k * tb * 2, mv, tb * 2, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(w.has_dev + k * tb, has, tb, hipMemcpyHostToDevice, stream));
    return PFV_OK;
}

constexpr int kDecWindows = 4;           // pfv_decoder: windows in flight -- the packet being decoded and up to three behind it
struct pfv_decoder {
    DecEntd entd;                        // switches, shape and counters of the device entropy stage (its buffers: win[])
    DecWindow win[kDecWindows];
    ListStage hp;                        // a packet the device stage left to the host parser
    hipStream_t win_stream = nullptr;
    pfv_ctx *ctx = nullptr;
    pfv_dec_session *hot = nullptr;
    const uint8_t *data = nullptr;
    size_t len = 0, pos = 0, reset_pos = 0;
    int width = 0, height = 0, framerate = 0, n_qtables = 0, total_blocks = 0;
    bool eof = false;
    double delta_accum = 0.0;
    PinnedBuf<uint8_t> retframe;           // Y|U|V, unpadded (src/dec.rs:22)
    uint8_t *frame_dev = nullptr;          // pfv_decoder_set_output_device: the retframe in device memory instead
    bool rgb_on = false;                   // pfv_decoder_set_output_rgb: the callback gets one tight picture in rgb_format instead of the planes
    int rgb_format = 0;
    PinnedBuf<uint8_t> rgbframe;           // ... in host memory
    uint8_t *rgb_dev = nullptr;            // ... in device memory (while frame_dev is set, and wherever the picture is made from a resized frame)
    size_t rgb_dev_cap = 0;
    // pfv_decoder_set_output_size: the callback gets the frame resized to out_w x out_h (and, with rgb_on, the picture of that frame)
    pfv_scaler *scaler = nullptr;          // width x height -> out_w x out_h; owned
    int out_w = 0, out_h = 0;
    uint8_t *scaled_dev = nullptr;         // one packed out_w x out_h frame in device memory: k_scale's destination
    PinnedBuf<uint8_t> scaledframe;        // ... and where it lands in host memory
    // look-ahead: ring of events in stream order, [head, head + count)
    std::vector<std::unique_ptr<DecEvent>> ring;
    size_t head = 0, count = 0;
    size_t scan_pos = 0;
    bool scan_stop = false;                // an END / ERROR event is pending: nothing is scanned past it
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    bool quit = false;
};

extern "C" {

// Encoder::new (src/enc.rs:37-73): q-tables from quality, prev_frame = new_padded, write_header (:190-219) -- for a ladder of qualities: the
// header carries 4 * n_rungs tables, rung-major, each rung in the order intra_l, intra_c, inter_l, inter_c
PFV_API int pfv_encoder_create_ladder(pfv_ctx *ctx, int width, int height, int framerate, const int *qualities, int n_rungs, pfv_encoder **out)
{
    if (!ctx || !out) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_encoder_create: bad argument");
    *out = nullptr;
    if (framerate < 0 || framerate > 65535) return fail(ctx, PFV_ERR_BAD_ARG, "framerate must fit u16 (src/enc.rs:197)");
    pfv_enc_session *hot = nullptr;
    int rc = pfv_enc_session_create_ladder(ctx, width, height, qualities, n_rungs, 1, &hot);
    if (rc) return rc;
    pfv_encoder *e = new pfv_encoder();
    e->ctx = ctx; e->hot = hot; e->width = width; e->height = height; e->framerate = framerate;
    e->total_blocks = pfv_total_blocks(width, height);
    if (!e->frame.resize(pfv_frame_bytes(width, height))) {
        pfv_encoder_destroy(e);
        return fail(ctx, PFV_ERR_NOMEM, "pfv_encoder_create: pinned staging");
    }
    put_header(e->out, width, height, framerate, qualities, n_rungs);
    *out = e;
    return PFV_OK;
}
PFV_API int pfv_encoder_create(pfv_ctx *ctx, int width, int height, int framerate, int quality, pfv_encoder **out)
{
    return pfv_encoder_create_ladder(ctx, width, height, framerate, &quality, 1, out);
}
// the rung of the frames that follow, on both entropy paths
PFV_API int pfv_encoder_set_rung(pfv_encoder *e, int rung)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    return pfv_enc_session_set_rung(e->hot, rung);
}
// the rung of the last frame written; before the first frame the current rung
PFV_API int pfv_encoder_rung(pfv_encoder *e)
{
    if (!e) return PFV_ERR_BAD_ARG;
    return e->last_rung >= 0 ? e->last_rung : e->hot->rung;
}
PFV_API int pfv_encoder_rungs(pfv_encoder *e) { return e ? e->hot->n_rungs : PFV_ERR_BAD_ARG; }
// p-frame byte budget per payload, 0 = off; the rule is at the declaration (include/pfv_hip_ext.h) and in rate_frame_written
PFV_API int pfv_encoder_set_rate(pfv_encoder *e, uint32_t pframe_budget)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    e->budget_p = pframe_budget;
    return PFV_OK;
}

// i-frame byte budget per payload, 0 = off; the rule is at the declaration (include/pfv_hip_ext.h) and in choose_iframe_rung
PFV_API int pfv_encoder_set_iframe_budget(pfv_encoder *e, uint32_t iframe_budget)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    e->budget_i = iframe_budget;
    return PFV_OK;
}

// i-frame quality floor in dB of PSNR-YUV, 0 = off; the rule is at the declaration (include/pfv_hip_ext.h) and in floor_rung
PFV_API int pfv_encoder_set_iframe_quality_floor(pfv_encoder *e, double min_psnr_yuv)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!(min_psnr_yuv >= 0.0)) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_iframe_quality_floor: the floor must be >= 0 dB (+INFINITY is legal, NaN is not)");
    e->floor_i = min_psnr_yuv;
    return PFV_OK;
}

// p-frame quality floor in dB of PSNR-YUV, 0 = off; the rules are at the declaration (include/pfv_hip_ext.h), in floor_rung and in
// pfv_encoder_encode_frame
PFV_API int pfv_encoder_set_pframe_quality_floor(pfv_encoder *e, double min_psnr_yuv)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!(min_psnr_yuv >= 0.0)) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_pframe_quality_floor: the floor must be >= 0 dB (+INFINITY is legal, NaN is not)");
    if (min_psnr_yuv > 0.0 && !enc_fourstep(e->hot)) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_set_pframe_quality_floor: the p-frame probes follow the four-step search only");
    e->floor_p = min_psnr_yuv;
    return PFV_OK;
}
// SSIM floors on the frame's mean SSIM (pfv_frame_ssim.ssim_all), 0 = off, (0, 1] legal; the rules are at the declarations
// (include/pfv_hip_ext.h), in ssim_floor_rung and in pfv_encoder_encode_frame
PFV_API int pfv_encoder_set_iframe_ssim_floor(pfv_encoder *e, double min_ssim)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!(min_ssim >= 0.0 && min_ssim <= 1.0)) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_iframe_ssim_floor: the floor must lie in [0, 1] (NaN is not legal)");
    e->sfloor_i = min_ssim;
    return PFV_OK;
}
PFV_API int pfv_encoder_set_pframe_ssim_floor(pfv_encoder *e, double min_ssim)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!(min_ssim >= 0.0 && min_ssim <= 1.0)) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_pframe_ssim_floor: the floor must lie in [0, 1] (NaN is not legal)");
    if (min_ssim > 0.0 && !enc_fourstep(e->hot)) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_set_pframe_ssim_floor: the p-frame probes follow the four-step search only");
    e->sfloor_p = min_ssim;
    return PFV_OK;
}
// a p-frame floor of either kind applies: it is set and there is a rung to choose
static bool pframe_floor(const pfv_encoder *e) { return (e->floor_p > 0.0 || e->sfloor_p > 0.0) && e->hot->n_rungs > 1; }

// the report of the encode_* call that has just written `packet_bytes` bytes (type 3: a drop frame, nothing measured)
static void fill_ssim(pfv_encoder *e, int type);
static void fill_report(pfv_encoder *e, int type, size_t packet_bytes)
{
    fill_ssim(e, type);
    if (!e->report_on) return;
    pfv_frame_report &r = e->report;
    const uint64_t ny = (uint64_t)e->width * (uint64_t)e->height, nc = (uint64_t)(e->width / 2) * (uint64_t)(e->height / 2);
    r.type = type;
    r.packet_bytes = (uint32_t)packet_bytes;
    for (int i = 0; i < 3; i++) {
        r.sse[i] = type == 3 ? 0 : e->sums.data()[i];
        r.psnr[i] = pfv_psnr(r.sse[i], i ? nc : ny);
    }
    r.psnr_yuv = pfv_psnr(r.sse[0] + r.sse[1] + r.sse[2], ny + 2 * nc);
    e->report_state = 1;
}

// the frame SSIM of the same call (type 3: a drop frame, nothing measured: zeros, and the value of identical frames)
static void fill_ssim(pfv_encoder *e, int type)
{
    if (!e->ssim_on) return;
    pfv_frame_ssim &r = e->ssim;
    (void)pfv_ssim_windows(e->width, e->height, r.windows);
    int64_t all = 0;
    uint64_t n_all = 0;
    for (int i = 0; i < 3; i++) {
        r.q24[i] = type == 3 ? 0 : e->ssim_sums.data()[i];
        r.ssim[i] = type == 3 ? 1.0 : pfv_ssim(r.q24[i], r.windows[i]);
        all += r.q24[i];
        n_all += r.windows[i];
    }
    r.ssim_all = type == 3 ? 1.0 : pfv_ssim(all, n_all);
    e->ssim_state = 1;
}

// the (y, u, v) of an entry point: three planes, or under pfv_encoder_set_input_rgb one picture as y with u == v == NULL
static bool planes_given(const pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v) { return e->rgb_on ? (y && !u && !v) : (y && u && v); }
static int upload_planes(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v);

static int pack_frame(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
    if (!planes_given(e, y, u, v)) return fail(e->ctx, PFV_ERR_BAD_ARG, e->rgb_on ? "RGB input is on: y is the picture, u and v must be NULL" : "null plane");
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:80)");
    if ((e->rgb_on || e->scaler || e->dn_on || e->sc_on) && !e->device_entropy) {   // the host entropy path takes its frame from `frame`: the converted / resized / filtered (and measured) planes come back down
        pfv_ctx *ctx = e->ctx;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        int rc = enc_staging(e->hot);
        if (!rc) rc = upload_planes(e, y, u, v);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(e->frame.data(), e->hot->st_frames, pfv_frame_bytes(e->width, e->height), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return PFV_OK;
    }
    if (e->device_entropy) {   // the planes go up from where they lie (encode_on_device): no packing copy -- it was half of a 4K frame's time
        e->plane[0] = y; e->plane[1] = u; e->plane[2] = v;
        return PFV_OK;
    }
    size_t ny = (size_t)e->width * e->height, nc = (size_t)(e->width / 2) * (e->height / 2);
    memcpy(e->frame.data(), y, ny);
    memcpy(e->frame.data() + ny, u, nc);
    memcpy(e->frame.data() + ny + nc, v, nc);
    return PFV_OK;
}

static int host_entropy_staging(pfv_encoder *e)
{
    if (e->coef.resize((size_t)e->total_blocks * 256) && e->mv.resize((size_t)e->total_blocks * 2) && e->has.resize((size_t)e->total_blocks))
        return PFV_OK;
    return fail(e->ctx, PFV_ERR_NOMEM, "pinned staging for the host entropy path");
}

// a frame's packet has been written at the session's current rung with `payload_bytes` of payload
static void rate_frame_written(pfv_encoder *e, bool pframe, size_t payload_bytes)
{
    pfv_enc_session *s = e->hot;
    e->last_rung = s->rung;
    e->n_written++;
    e->since_iframe = pframe ? e->since_iframe + 1 : 0;
    // with the probe or the p-frame floor on the budget is the hard one: the rung was chosen before the frame was written
    if (!pframe || !e->budget_p || e->pprobe_on || pframe_floor(e)) return;
    if (payload_bytes > e->budget_p) s->rung = std::min(s->rung + 1, s->n_rungs - 1);
    else if (2 * (uint64_t)payload_bytes <= e->budget_p) s->rung = std::max(s->rung - 1, 0);
}

// the planes into the session's frame staging (which exists), on the context's stream: read until the caller's next synchronisation
static int upload_planes(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
    pfv_enc_session *s = e->hot;
    pfv_ctx *ctx = e->ctx;
    // the filter's state moves once per frame: the entry point's first upload runs it, the frame then lies in the staging for the rest of the call
    if ((e->dn_on || e->sc_on) && e->dn_staged) return PFV_OK;
    // what the caller hands over has the size iw x ih; its planar form goes to `planar`: the staging itself, or where it waits for k_scale or
    // k_denoise; `sized`: where the frame of the session's size goes
    const int iw = e->scaler ? e->src_w : e->width, ih = e->scaler ? e->src_h : e->height;
    const size_t ny = (size_t)iw * ih, nc = (size_t)(iw / 2) * (ih / 2), fb = (size_t)s->geom.src_frame_bytes;
    uint8_t *sized = e->dn_on ? e->dn_src : s->st_frames;
    uint8_t *planar = e->scaler ? e->scale_src : sized;
    if (e->rgb_on) {   // the picture up into the encoder's scratch, one k_ingest_rgb
        const size_t row = pfv_rgb_row_bytes(iw, e->rgb_format);
        hipError_t he = hipMemcpyAsync(e->rgb_scratch, y, row * (size_t)ih, hipMemcpyHostToDevice, ctx->stream);
        if (he != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return hip_fail(ctx, he, "picture upload"); }
        const int rc = ingest_launch(ctx, iw, ih, 1, e->rgb_scratch, e->rgb_format, row, row * (size_t)ih, planar, ny + 2 * nc, e->rgb_chroma);
        if (rc) return rc;
    } else {
        const bool packed = u == y + ny && v == u + nc;   // a packed frame: one copy
        hipError_t he = hipMemcpyAsync(planar, y, packed ? ny + 2 * nc : ny, hipMemcpyHostToDevice, ctx->stream);
        if (!packed && he == hipSuccess) he = hipMemcpyAsync(planar + ny, u, nc, hipMemcpyHostToDevice, ctx->stream);
        if (!packed && he == hipSuccess) he = hipMemcpyAsync(planar + ny + nc, v, nc, hipMemcpyHostToDevice, ctx->stream);
        if (he != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return hip_fail(ctx, he, "plane upload"); }
    }
    if (e->scaler) {   // one k_scale into the staging, or to where the frame waits for k_denoise
        const int rc = scale_launch(e->scaler, 1, e->scale_src, PFV_FRAME_PACKED, ny + 2 * nc, sized, fb);
        if (rc) return rc;
    }
    if (e->dn_on) {   // one k_denoise into the staging
        const int rc = denoise_launch(e->dn, 0, 1, e->dn_src, PFV_FRAME_PACKED, fb, s->st_frames, fb, e->dn_commit ? 1 : 0, "pfv_encoder");
        if (rc) return rc;
    }
    if (e->sc_on) {   // the staged frame measured against the detector's state: one launch group, the 40 bytes on their way down
        const int rc = scene_launch(e->sc, 0, 1, 0, s->st_frames, PFV_FRAME_PACKED, 0, e->dn_commit ? 1 : 0, e->sc_dev, "pfv_encoder");
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(e->sc_host.data(), e->sc_dev, sizeof(pfv_scene_stats), hipMemcpyDeviceToHost, ctx->stream));
        e->sc_measured = true;
    }
    if (e->dn_on || e->sc_on) e->dn_staged = true;
    return PFV_OK;
}

// One frame through the device entropy stage: planes up (unless the i-frame budget's probe has put them there: `staged`), kernels, payload size
// then payload bytes down.
static int encode_on_device(pfv_encoder *e, bool pframe, bool staged = false)
{
    pfv_enc_session *s = e->hot;
    pfv_ctx *ctx = e->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = enc_staging(s);
    if (!rc) rc = pfv_enc_entropy_enable(s, 0);
    if (rc) return rc;
    // the caller's planes are read until the first synchronisation below (pfv_enc_payload_sizes); every exit before it synchronises too
    if (!staged && (rc = upload_planes(e, e->plane[0], e->plane[1], e->plane[2]))) return rc;
    rc = pframe ? pfv_enc_pframe_dev(s, s->st_frames, s->st_mv, s->st_has, s->st_coef) : pfv_enc_iframe_dev(s, s->st_frames, s->st_coef);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    // from here on prev_frame has moved to this frame: a failure leaves the encoder's reference ahead of the stream
    e->poisoned = true;
    if (e->report_on && (rc = enc_report_enqueue(s))) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // arrives with the payload size
    if (e->ssim_on && (rc = enc_ssim_enqueue(s))) { (void)hipStreamSynchronize(ctx->stream); return rc; }       // and so do these
    rc = pframe ? pfv_enc_pack_pframe_dev(s, s->st_mv, s->st_has, s->st_coef) : pfv_enc_pack_iframe_dev(s, s->st_coef);
    uint32_t nbytes = 0;
    if (!rc) rc = pfv_enc_payload_sizes(s, &nbytes);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    if (!e->payload.resize(std::max<size_t>(nbytes, 1 << 20))) return fail(ctx, PFV_ERR_NOMEM, "pinned payload staging");
    if ((rc = pfv_enc_payload_fetch(s, 0, e->payload.data(), nbytes))) return rc;
    e->poisoned = false;
    put_packet(e->out, pframe ? 2 : 1, e->payload.data(), nbytes);
    fill_report(e, pframe ? 2 : 1, 5 + (size_t)nbytes);
    rate_frame_written(e, pframe, nbytes);
    return PFV_OK;
}

// 1 (default): RLE + Huffman + bit packing on the device; 0: on the host (serialize_iframe / serialize_pframe).  The
// bytes written are the same either way.
PFV_API int pfv_encoder_set_device_entropy(pfv_encoder *e, int on)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    e->device_entropy = on != 0;
    return PFV_OK;
}

// the encoder's device scratch for the input switches that are on, at the size of what the caller hands over; made by the set calls only
static int enc_input_scratch(pfv_encoder *e)
{
    pfv_ctx *ctx = e->ctx;
    const int iw = e->scaler ? e->src_w : e->width, ih = e->scaler ? e->src_h : e->height;
    if (e->scaler && !e->scale_src) HIP_TRY(ctx, hipMalloc((void **)&e->scale_src, pfv_frame_bytes(iw, ih)));
    if (e->dn_on && !e->dn_src) HIP_TRY(ctx, hipMalloc((void **)&e->dn_src, pfv_frame_bytes(e->width, e->height)));
    const size_t pic = (size_t)iw * ih * 4;
    if (e->rgb_on && e->rgb_scratch_cap < pic) {
        if (e->rgb_scratch) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(e->rgb_scratch); e->rgb_scratch = nullptr; e->rgb_scratch_cap = 0; }
        HIP_TRY(ctx, hipMalloc((void **)&e->rgb_scratch, pic));
        e->rgb_scratch_cap = pic;
    }
    return PFV_OK;
}

// RGB picture input: while on, the (y, u, v) of every encode_* / probe_* call is (one tight picture in `format`, NULL, NULL); pack_frame and
// upload_planes are the two places a frame enters, and the only ones that know (include/pfv_hip_ext.h, "RGB / RGBA picture input")
PFV_API int pfv_encoder_set_input_rgb(pfv_encoder *e, int on, int format, int chroma)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!on) {
        e->rgb_on = false;
        return PFV_OK;
    }
    pfv_ctx *ctx = e->ctx;
    if (!pix_format_ok(format)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_input_rgb: format must be PFV_PIX_RGB8, _RGBA8 or _BGRA8");
    if (!chroma_mode_ok(chroma)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_input_rgb: chroma must be PFV_CHROMA_POINT or PFV_CHROMA_BOX");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = enc_staging(e->hot);
    if (rc) return rc;
    e->rgb_on = true; e->rgb_format = format; e->rgb_chroma = chroma;
    return enc_input_scratch(e);
}

// Resized input: while on, what every encode_* / probe_* call takes -- the planes, or under pfv_encoder_set_input_rgb the picture -- has the
// size src_w x src_h; it goes up into scratch of the encoder and one k_scale puts the frame into the session's frame staging (upload_planes)
PFV_API int pfv_encoder_set_input_size(pfv_encoder *e, int src_w, int src_h, int kind)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    pfv_ctx *ctx = e->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    pfv_scaler *sc = nullptr;
    if (src_w != 0) {
        int rc = PFV_OK;
        if (!(sc = pfv_scaler_create(ctx, src_w, src_h, e->width, e->height, kind, &rc))) return rc;
        if ((rc = enc_staging(e->hot))) { pfv_scaler_destroy(sc); return rc; }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // nothing reads the old tables or scratch any more
    pfv_scaler_destroy(e->scaler);
    if (e->scale_src) { (void)hipFree(e->scale_src); e->scale_src = nullptr; }
    e->scaler = sc;
    e->src_w = sc ? src_w : 0; e->src_h = sc ? src_h : 0;
    return enc_input_scratch(e);
}

// Denoising pre-filter: while on, the frame of the session's size -- as handed over, converted or resized -- waits in scratch of the encoder and
// one k_denoise puts it into the session's frame staging (upload_planes).  The encode_* calls commit, the probe_* calls do not.
PFV_API int pfv_encoder_set_denoise(pfv_encoder *e, int on, const uint8_t spatial[3], const uint8_t temporal[3])
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!on) {
        e->dn_on = false;
        return PFV_OK;
    }
    pfv_ctx *ctx = e->ctx;
    if (!spatial || !temporal) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_denoise: null strengths");
    if (!denoise_strengths_ok(spatial, temporal)) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_denoise: strength above 16");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = enc_staging(e->hot);
    if (rc) return rc;
    if (!e->dn && !(e->dn = pfv_denoiser_create(ctx, e->width, e->height, 1, &rc))) return rc;
    if (!e->dn_on && (rc = pfv_denoiser_reset(e->dn, 0, 1))) return rc;   // switched on: the filter starts without a past
    if ((rc = pfv_denoiser_set_strength(e->dn, spatial, temporal))) return rc;
    e->dn_on = true;
    return enc_input_scratch(e);
}

// Scene-cut detection: while on, upload_planes measures the staged frame once per entry point (the encode_* calls commit the detector's state,
// the probe_* calls do not) and pfv_encoder_encode_frame takes rule 1b from the score.
PFV_API int pfv_encoder_set_scene_cut(pfv_encoder *e, int on, uint32_t threshold_q8, int radius, int min_interval)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!on) {
        e->sc_on = false;
        return PFV_OK;
    }
    pfv_ctx *ctx = e->ctx;
    if (radius < 0 || radius > kSceneMaxR || min_interval < 0) return fail(ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_scene_cut: the radius is 0 .. 7, min_interval not negative");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = enc_staging(e->hot);
    if (rc) return rc;
    if (!e->sc && !(e->sc = pfv_scene_detector_create(ctx, e->width, e->height, 1, 0, &rc))) return rc;
    if (!e->sc_dev) HIP_TRY(ctx, hipMalloc((void **)&e->sc_dev, sizeof(pfv_scene_stats)));
    if (!e->sc_host.resize(1)) return fail(ctx, PFV_ERR_NOMEM, "pinned staging for the scene stats");
    if (!e->sc_on) {   // switched on: the detector starts without a past
        if ((rc = pfv_scene_detector_reset(e->sc, 0, 1))) return rc;
        e->sc_measured = false;
    }
    if ((rc = pfv_scene_detector_set_radius(e->sc, radius))) return rc;
    e->sc_threshold = threshold_q8;
    e->sc_min_interval = min_interval;
    e->sc_on = true;
    return PFV_OK;
}
PFV_API int pfv_encoder_last_scene(pfv_encoder *e, pfv_scene_stats *out)
{
    if (!e || !out) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_encoder_last_scene: bad argument");
    if (!e->sc_on || !e->sc_measured) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_last_scene: scene-cut detection is off or has measured no frame yet");
    HIP_TRY(e->ctx, hipSetDevice(e->ctx->device));
    HIP_TRY(e->ctx, hipStreamSynchronize(e->ctx->stream));   // an entry point that failed may have left the download in flight
    *out = *e->sc_host.data();
    return PFV_OK;
}

// Frame reports: with them on, every encode_* call also measures the frame it was given against the reconstruction it leaves in prev_frame
// (k_sse_mb + k_sse_sum behind the encode kernel) and keeps what it wrote; the stream bytes do not change.
PFV_API int pfv_encoder_set_frame_report(pfv_encoder *e, int on)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (on && !e->sums.resize(3)) return fail(e->ctx, PFV_ERR_NOMEM, "pinned staging for the frame reports");
    int rc = enc_report_enable(e->hot, on ? e->sums.data() : nullptr);
    if (rc) return rc;
    if (!on || !e->report_on) e->report_state = 0;
    e->report_on = on != 0;
    return PFV_OK;
}
PFV_API int pfv_encoder_frame_report(pfv_encoder *e, pfv_frame_report *out)
{
    if (!e || !out) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_encoder_frame_report: bad argument");
    if (!e->report_on) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_frame_report: reports are off (pfv_encoder_set_frame_report)");
    if (e->report_state == 0) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_frame_report: no frame has been encoded yet");
    if (e->report_state < 0) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_frame_report: the last encode call failed");
    *out = e->report;
    return PFV_OK;
}

// Frame SSIM: with it on, every encode_* call also measures the structural similarity between the frame it was given and the reconstruction
// it leaves in prev_frame (k_ssim_mb + k_ssim_sum behind the encode kernel); the stream bytes do not change.
PFV_API int pfv_encoder_set_frame_ssim(pfv_encoder *e, int on)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (on && !e->ssim_sums.resize(3)) return fail(e->ctx, PFV_ERR_NOMEM, "pinned staging for the frame SSIM");
    int rc = enc_ssim_enable(e->hot, on ? e->ssim_sums.data() : nullptr);
    if (rc) return rc;
    if (!on || !e->ssim_on) e->ssim_state = 0;
    e->ssim_on = on != 0;
    return PFV_OK;
}
PFV_API int pfv_encoder_frame_ssim(pfv_encoder *e, pfv_frame_ssim *out)
{
    if (!e || !out) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_encoder_frame_ssim: bad argument");
    if (!e->ssim_on) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_frame_ssim: frame SSIM is off (pfv_encoder_set_frame_ssim)");
    if (e->ssim_state == 0) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_frame_ssim: no frame has been encoded yet");
    if (e->ssim_state < 0) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_frame_ssim: the last encode call failed");
    *out = e->ssim;
    return PFV_OK;
}

// the finest rung whose probed payload fits `budget`: the scan starts at rung 0, a rung marked not encodable does not fit, the coarsest if none does
static int budget_rung(const pfv_enc_session *s, const uint32_t *sizes, uint32_t budget)
{
    for (int r = 0; r < s->n_rungs; r++)
        if (sizes[r] != kEntErrOversize && sizes[r] <= budget) return r;
    return s->n_rungs - 1;
}
// A quality floor's rung (the i-frame's or the p-frame's, each with its own budget, 0: none) from the probed sizes and plane sums
// [n_rungs][3].  Allowed: encodable and, under a budget, within it.  Of the allowed rungs whose PSNR-YUV (pfv_frame_report's) reaches the floor the one with the fewest bytes; if none does, the allowed rung
// with the smallest squared error, then the fewest bytes; ties to the lower index.  No rung allowed: the coarsest, as budget_rung.
static int floor_rung(const pfv_encoder *e, const uint32_t *sizes, const uint64_t *sse, uint32_t budget, double floor_db)
{
    const pfv_enc_session *s = e->hot;
    const uint64_t samples = (uint64_t)pfv_frame_bytes(e->width, e->height);
    int meets = -1, best = -1;
    uint64_t best_sse = 0;
    for (int r = 0; r < s->n_rungs; r++) {
        if (sizes[r] == kEntErrOversize || (budget && sizes[r] > budget)) continue;
        const uint64_t total = sse[3 * r] + sse[3 * r + 1] + sse[3 * r + 2];
        if (pfv_psnr(total, samples) >= floor_db && (meets < 0 || sizes[r] < sizes[meets])) meets = r;
        if (best < 0 || total < best_sse || (total == best_sse && sizes[r] < sizes[best])) { best = r; best_sse = total; }
    }
    return meets >= 0 ? meets : best >= 0 ? best : s->n_rungs - 1;
}
// windows of the whole frame (pfv_ssim_windows over the three planes)
static uint64_t frame_windows(const pfv_encoder *e)
{
    uint32_t n[3] = {0, 0, 0};
    (void)pfv_ssim_windows(e->width, e->height, n);
    return (uint64_t)n[0] + n[1] + n[2];
}
// a candidate meets the floors that are on (0: off) with its plane sums of squared error and of q; a frame without windows meets every SSIM floor
static bool meets_floors(const pfv_encoder *e, const uint64_t *sse, const int64_t *q24, double floor_db, double floor_ssim)
{
    if (floor_db > 0.0 && !(pfv_psnr(sse[0] + sse[1] + sse[2], (uint64_t)pfv_frame_bytes(e->width, e->height)) >= floor_db)) return false;
    const uint64_t windows = frame_windows(e);
    return !(floor_ssim > 0.0) || windows == 0 || pfv_ssim(q24[0] + q24[1] + q24[2], windows) >= floor_ssim;
}
// floor_rung with an SSIM floor beside the PSNR floor (either may be 0: off; with the SSIM floor off it IS floor_rung): sizes, plane sums
// [n_rungs][3] and SSIM sums [n_rungs][3] of the SSIM probe.  Allowed as there.  Of the allowed rungs that meet both floors the one with the
// fewest bytes; if none does and the frame has windows, the allowed rung with the largest q24 total, then the smallest squared error, then
// the fewest bytes; ties to the lower index.  Without windows the SSIM floor is met by every rung and floor_rung's answer holds.
static int ssim_floor_rung(const pfv_encoder *e, const uint32_t *sizes, const uint64_t *sse, const int64_t *q24, uint32_t budget, double floor_db, double floor_ssim)
{
    const pfv_enc_session *s = e->hot;
    if (!(floor_ssim > 0.0) || frame_windows(e) == 0) {
        if (floor_db > 0.0) return floor_rung(e, sizes, sse, budget, floor_db);
        int meets = -1;   // no floor decides: the fewest bytes of the allowed rungs
        for (int r = 0; r < s->n_rungs; r++)
            if (sizes[r] != kEntErrOversize && !(budget && sizes[r] > budget) && (meets < 0 || sizes[r] < sizes[meets])) meets = r;
        return meets >= 0 ? meets : s->n_rungs - 1;
    }
    int meets = -1, best = -1;
    int64_t best_q = 0;
    uint64_t best_sse = 0;
    for (int r = 0; r < s->n_rungs; r++) {
        if (sizes[r] == kEntErrOversize || (budget && sizes[r] > budget)) continue;
        const uint64_t total = sse[3 * r] + sse[3 * r + 1] + sse[3 * r + 2];
        const int64_t q = q24[3 * r] + q24[3 * r + 1] + q24[3 * r + 2];
        if (meets_floors(e, sse + 3 * r, q24 + 3 * r, floor_db, floor_ssim) && (meets < 0 || sizes[r] < sizes[meets])) meets = r;
        if (best < 0 || q > best_q || (q == best_q && (total < best_sse || (total == best_sse && sizes[r] < sizes[best])))) { best = r; best_q = q; best_sse = total; }
    }
    return meets >= 0 ? meets : best >= 0 ? best : s->n_rungs - 1;
}
// The i-frame byte budget: the frame goes up into the session's staging, the probe sizes it at every rung, and the finest rung whose payload
// fits becomes the current rung (the coarsest if none does; a rung the probe marks not encodable does not fit).  With a quality floor the
// rate-distortion probe runs in its place and floor_rung chooses.
// staged: the frame lies in the session's staging already; probed: ... and these are its i-frame sizes (pfv_encoder_encode_frame)
static int choose_iframe_rung(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, bool staged, const uint32_t *probed)
{
    pfv_enc_session *s = e->hot;
    HIP_TRY(e->ctx, hipSetDevice(e->ctx->device));
    int rc = enc_staging(s);
    if (!rc && !staged) rc = upload_planes(e, y, u, v);
    uint32_t sizes[kMaxRungs];
    if (e->sfloor_i > 0.0) {   // the SSIM probe in the RD probe's place
        uint64_t sse[kMaxRungs][3];
        int64_t q24[kMaxRungs][3];
        if (!rc) rc = ssim_probe_staged(s, false, sizes, &sse[0][0], &q24[0][0]);
        if (rc) return rc;
        s->rung = ssim_floor_rung(e, sizes, &sse[0][0], &q24[0][0], e->budget_i, e->floor_i, e->sfloor_i);
        return PFV_OK;
    }
    if (e->floor_i > 0.0) {
        uint64_t sse[kMaxRungs][3];
        if (!rc) rc = rd_probe_staged(s, sizes, &sse[0][0]);
        if (rc) return rc;
        s->rung = floor_rung(e, sizes, &sse[0][0], e->budget_i, e->floor_i);
        return PFV_OK;
    }
    if (!rc && !probed) rc = probe_staged(s, sizes);
    if (rc) return rc;
    s->rung = budget_rung(s, probed ? probed : sizes, e->budget_i);
    return PFV_OK;
}

// an i-frame budget or floor applies: encode_iframe probes and chooses its rung
static bool iframe_rung_rule(const pfv_encoder *e) { return (e->budget_i != 0 || e->floor_i > 0.0 || e->sfloor_i > 0.0) && e->hot->n_rungs > 1; }   // one rung: nothing to choose

// Encoder::encode_iframe (src/enc.rs:75-123) behind pack_frame.  staged / probed: see choose_iframe_rung; settled: the frame lies in the staging
// and the current rung is the one to write at (pfv_encoder_encode_frame under the p-frame floor)
static int write_iframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, bool staged = false, const uint32_t *probed = nullptr,
                        bool settled = false)
{
    int rc;
    const bool budget = !settled && iframe_rung_rule(e);
    if (budget && (rc = choose_iframe_rung(e, y, u, v, staged, probed))) return rc;
    staged = staged || budget;
    if (e->device_entropy) return encode_on_device(e, false, staged);      // an i-frame replaces prev_frame entirely: clears a poisoned state
    if ((rc = host_entropy_staging(e))) return rc;
    if ((rc = enc_iframe_host(e->hot, staged ? nullptr : e->frame.data(), e->coef.data()))) return rc;
    e->poisoned = true;
    std::vector<uint8_t> payload;
    const uint8_t qidx[3] = {(uint8_t)(4 * e->hot->rung), (uint8_t)(4 * e->hot->rung + 1), (uint8_t)(4 * e->hot->rung + 1)};
    if (!serialize_iframe(payload, e->coef.data(), e->total_blocks, qidx))
        return fail(e->ctx, PFV_ERR_FORMAT, "coefficient needs more than 15 size bits (src/rle.rs:44)");
    put_packet(e->out, 1, payload.data(), payload.size());
    e->poisoned = false;
    fill_report(e, 1, 5 + payload.size());
    rate_frame_written(e, false, payload.size());
    return PFV_OK;
}
PFV_API int pfv_encoder_encode_iframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->report_on) e->report_state = -1;   // until this call has written its packet
    if (e->ssim_on) e->ssim_state = -1;
    e->dn_commit = true; e->dn_staged = false;   // the frame this call uploads moves the filter's state
    int rc = pack_frame(e, y, u, v);
    if (rc) return rc;
    return write_iframe(e, y, u, v);
}
// payload bytes of this frame as an i-frame at every rung; the encoder's stream, reference and rung stay as they are
PFV_API int pfv_encoder_probe_iframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!planes_given(e, y, u, v) || !sizes_out) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_probe_iframe: null buffer");
    HIP_TRY(e->ctx, hipSetDevice(e->ctx->device));
    e->dn_commit = false; e->dn_staged = false;   // a probe leaves the filter's state alone
    int rc = enc_staging(e->hot);
    if (!rc) rc = upload_planes(e, y, u, v);
    if (!rc) rc = probe_staged(e->hot, sizes_out);
    return rc;
}
// ... and its squared error per plane at every rung [n_rungs][3], from the same read of the frame
PFV_API int pfv_encoder_probe_iframe_rd(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out, uint64_t *sse_out)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!planes_given(e, y, u, v) || !sizes_out || !sse_out) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_probe_iframe_rd: null buffer");
    HIP_TRY(e->ctx, hipSetDevice(e->ctx->device));
    e->dn_commit = false; e->dn_staged = false;   // a probe leaves the filter's state alone
    int rc = enc_staging(e->hot);
    if (!rc) rc = upload_planes(e, y, u, v);
    if (!rc) rc = rd_probe_staged(e->hot, sizes_out, sse_out);
    return rc;
}
// ... and its SSIM sums per plane at every rung [n_rungs][3], from the same read of the frame
PFV_API int pfv_encoder_probe_iframe_ssim(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out, uint64_t *sse_out, int64_t *ssim_q24_out)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!planes_given(e, y, u, v) || !sizes_out || !sse_out || !ssim_q24_out) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_probe_iframe_ssim: null buffer");
    HIP_TRY(e->ctx, hipSetDevice(e->ctx->device));
    e->dn_commit = false; e->dn_staged = false;   // a probe leaves the filter's state alone
    int rc = enc_staging(e->hot);
    if (!rc) rc = upload_planes(e, y, u, v);
    if (!rc) rc = ssim_probe_staged(e->hot, false, sizes_out, sse_out, ssim_q24_out);
    return rc;
}
// the frame up into the session's staging and sized as a p-frame at every rung (counts: [n_rungs][kPProbeStats], or nullptr); sse
// ([n_rungs][3], or nullptr): the rate-distortion probe in the size probe's place; q24 ([n_rungs][3], or nullptr; with sse): the SSIM probe
static int probe_pframe_planes(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes, uint32_t *counts, uint64_t *sse = nullptr,
                               int64_t *q24 = nullptr)
{
    if (int rf = enc_pframe_probe_refused(e->hot, "pfv_encoder_probe_pframe")) return rf;
    HIP_TRY(e->ctx, hipSetDevice(e->ctx->device));
    int rc = enc_staging(e->hot);
    if (!rc) rc = upload_planes(e, y, u, v);
    if (!rc) rc = q24 ? ssim_probe_staged(e->hot, true, sizes, sse, q24, counts) : sse ? prd_probe_staged(e->hot, sizes, sse, counts) : pprobe_staged(e->hot, sizes, counts);
    return rc;
}
// payload bytes of this frame as a p-frame against the encoder's reference at every rung; the stream, the reference and the rung stay as they are
PFV_API int pfv_encoder_probe_pframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!planes_given(e, y, u, v) || !sizes_out) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_probe_pframe: null buffer");
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:80)");
    if (e->poisoned) return fail(e->ctx, PFV_ERR_STATE, "the previous frame failed after prev_frame had advanced: encode an i-frame next");
    e->dn_commit = false; e->dn_staged = false;   // a probe leaves the filter's state alone
    return probe_pframe_planes(e, y, u, v, sizes_out, nullptr);
}
// ... and its squared error per plane at every rung [n_rungs][3], from the same search and transform
PFV_API int pfv_encoder_probe_pframe_rd(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out, uint64_t *sse_out)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!planes_given(e, y, u, v) || !sizes_out || !sse_out) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_probe_pframe_rd: null buffer");
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:80)");
    if (e->poisoned) return fail(e->ctx, PFV_ERR_STATE, "the previous frame failed after prev_frame had advanced: encode an i-frame next");
    e->dn_commit = false; e->dn_staged = false;   // a probe leaves the filter's state alone
    return probe_pframe_planes(e, y, u, v, sizes_out, nullptr, sse_out);
}
// ... and its SSIM sums per plane at every rung [n_rungs][3]
PFV_API int pfv_encoder_probe_pframe_ssim(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out, uint64_t *sse_out, int64_t *ssim_q24_out)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!planes_given(e, y, u, v) || !sizes_out || !sse_out || !ssim_q24_out) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_probe_pframe_ssim: null buffer");
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:80)");
    if (e->poisoned) return fail(e->ctx, PFV_ERR_STATE, "the previous frame failed after prev_frame had advanced: encode an i-frame next");
    e->dn_commit = false; e->dn_staged = false;   // a probe leaves the filter's state alone
    return probe_pframe_planes(e, y, u, v, sizes_out, nullptr, sse_out, ssim_q24_out);
}
PFV_API int pfv_encoder_set_pframe_probe(pfv_encoder *e, int on)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (on && !enc_fourstep(e->hot)) return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_set_pframe_probe: the p-frame probes follow the four-step search only");
    e->pprobe_on = on != 0;
    return PFV_OK;
}
// the motion search of the p-frames that follow (the hot session's mode); refused while anything that probes p-frames is on
PFV_API int pfv_encoder_set_motion_search(pfv_encoder *e, int mode, int radius)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    const bool valid = (mode == PFV_SEARCH_FULL && radius >= 1 && radius <= 15) || (mode == PFV_SEARCH_HIER && radius >= 2 && radius <= 62 && !(radius & 1));
    if (valid && (e->pprobe_on || e->floor_p > 0.0 || e->sfloor_p > 0.0))
        return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_set_motion_search: the p-frame probe and the p-frame floors follow the four-step search only: switch them off first");
    return pfv_enc_session_set_motion_search(e->hot, mode, radius);
}
PFV_API int pfv_encoder_set_gop(pfv_encoder *e, int max_interval)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (max_interval < 0) return fail(e->ctx, PFV_ERR_BAD_ARG, "pfv_encoder_set_gop: max_interval must be >= 0");
    e->gop_max = max_interval;
    return PFV_OK;
}
// the hard p-frame budget applies: the probe is on, a budget is set and there is a rung to choose
static bool hard_pframe_budget(const pfv_encoder *e) { return e->pprobe_on && e->budget_p != 0 && e->hot->n_rungs > 1; }

// Encoder::encode_pframe (src/enc.rs:125-173) behind pack_frame and the poisoned test.  staged: the frame lies in the session's staging and the
// rung is settled (pfv_encoder_encode_frame); otherwise the p-frame floor or the hard budget, where one applies, probes the frame and chooses
// the rung first (the floor's rule takes the budget in as a hard cap).
static int write_pframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, bool staged = false)
{
    int rc;
    if (!staged && pframe_floor(e) && e->sfloor_p > 0.0) {   // the SSIM probe in the RD probe's place
        uint32_t sizes[kMaxRungs];
        uint64_t sse[kMaxRungs][3];
        int64_t q24[kMaxRungs][3];
        if ((rc = probe_pframe_planes(e, y, u, v, sizes, nullptr, &sse[0][0], &q24[0][0]))) return rc;
        e->hot->rung = ssim_floor_rung(e, sizes, &sse[0][0], &q24[0][0], e->budget_p, e->floor_p, e->sfloor_p);
        staged = true;
    } else if (!staged && pframe_floor(e)) {
        uint32_t sizes[kMaxRungs];
        uint64_t sse[kMaxRungs][3];
        if ((rc = probe_pframe_planes(e, y, u, v, sizes, nullptr, &sse[0][0]))) return rc;
        e->hot->rung = floor_rung(e, sizes, &sse[0][0], e->budget_p, e->floor_p);
        staged = true;
    } else if (!staged && hard_pframe_budget(e)) {
        uint32_t sizes[kMaxRungs];
        if ((rc = probe_pframe_planes(e, y, u, v, sizes, nullptr))) return rc;
        e->hot->rung = budget_rung(e->hot, sizes, e->budget_p);
        staged = true;
    }
    if (e->device_entropy) return encode_on_device(e, true, staged);
    if ((rc = host_entropy_staging(e))) return rc;
    if ((rc = enc_pframe_host(e->hot, staged ? nullptr : e->frame.data(), e->mv.data(), e->has.data(), e->coef.data()))) return rc;
    e->poisoned = true;
    std::vector<uint8_t> payload;
    const uint8_t qidx[3] = {(uint8_t)(4 * e->hot->rung + 2), (uint8_t)(4 * e->hot->rung + 3), (uint8_t)(4 * e->hot->rung + 3)};
    if (!serialize_pframe(payload, e->mv.data(), e->has.data(), e->coef.data(), e->total_blocks, qidx))
        return fail(e->ctx, PFV_ERR_FORMAT, "coefficient needs more than 15 size bits (src/rle.rs:44)");
    put_packet(e->out, 2, payload.data(), payload.size());
    e->poisoned = false;
    fill_report(e, 2, 5 + payload.size());
    rate_frame_written(e, true, payload.size());
    return PFV_OK;
}
PFV_API int pfv_encoder_encode_pframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->report_on) e->report_state = -1;   // until this call has written its packet
    if (e->ssim_on) e->ssim_state = -1;
    e->dn_commit = true; e->dn_staged = false;   // the frame this call uploads moves the filter's state
    int rc = pack_frame(e, y, u, v);
    if (rc) return rc;
    // a previous frame failed after the encoder's reference had advanced but before its packet was written: a p-frame
    // now would predict from a frame the decoder never saw (the reference panics in that situation and the Encoder is gone)
    if (e->poisoned) return fail(e->ctx, PFV_ERR_STATE, "the previous frame failed after prev_frame had advanced: encode an i-frame next");
    return write_pframe(e, y, u, v);
}
static void write_dropframe(pfv_encoder *e)
{
    put_packet(e->out, 1, nullptr, 0);
    fill_report(e, 3, 5);
    e->n_written++;
    e->since_iframe++;
}
// Rule 4 of pfv_encoder_encode_frame under the p-frame floor: the p-frame at rp against the i-frame at ri, each with its probed payload bytes
// and plane sums.  A candidate meets when its PSNR-YUV reaches the P-FRAME floor; exactly one meets: that one; both: fewer bytes, ties to the
// i-frame; neither: the smaller squared error, then fewer bytes, then the i-frame.  A candidate that is not encodable (its sums are undefined)
// never meets and loses to one that is; neither encodable: the i-frame, as today's rule.
// pq / iq: the candidates' SSIM sums where the SSIM probe measured them (nullptr: the RD probe did; the p-frame SSIM floor is then off).  A
// candidate meets when it meets every P-FRAME floor that is on; neither meets under the p-frame SSIM floor, in a frame that has windows: the
// larger q24 total decides before the squared error.
static bool rd_prefers_iframe(const pfv_encoder *e, uint32_t pbytes, const uint64_t (&psse)[3], uint32_t ibytes, const uint64_t (&isse)[3],
                              const int64_t *pq = nullptr, const int64_t *iq = nullptr)
{
    if (ibytes == kEntErrOversize || pbytes == kEntErrOversize) return pbytes == kEntErrOversize;
    const uint64_t pt = psse[0] + psse[1] + psse[2], it = isse[0] + isse[1] + isse[2];
    const double sfloor = pq && iq ? e->sfloor_p : 0.0;
    const bool pm = meets_floors(e, psse, pq, e->floor_p, sfloor), im = meets_floors(e, isse, iq, e->floor_p, sfloor);
    if (pm != im) return im;
    if (pm) return ibytes <= pbytes;
    if (sfloor > 0.0 && frame_windows(e) != 0) {
        const int64_t pqt = pq[0] + pq[1] + pq[2], iqt = iq[0] + iq[1] + iq[2];
        if (pqt != iqt) return iqt > pqt;
    }
    return it != pt ? it < pt : ibytes <= pbytes;
}
// The frame's type chosen by the probes; the rules, in this order, are at the declaration (include/pfv_hip_ext.h)
PFV_API int pfv_encoder_encode_frame(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, int *type_out)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (!e->sc_on && !enc_fourstep(e->hot))
        return fail(e->ctx, PFV_ERR_STATE, "pfv_encoder_encode_frame: the frame type comes from the p-frame probes, which follow the four-step search only (or from pfv_encoder_set_scene_cut)");
    if (e->report_on) e->report_state = -1;   // until this call has written its packet
    if (e->ssim_on) e->ssim_state = -1;
    e->dn_commit = true; e->dn_staged = false;   // the frame this call uploads moves the filter's state
    int rc = pack_frame(e, y, u, v);
    if (rc) return rc;
    pfv_enc_session *s = e->hot;
    int type = 1;
    bool cut = false;
    if (e->sc_on) {   // the frame up and measured before anything is decided (the host entropy path did both in pack_frame)
        pfv_ctx *ctx = e->ctx;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (e->device_entropy) {
            rc = enc_staging(s);
            if (!rc) rc = upload_planes(e, y, u, v);
            if (rc) return rc;
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        cut = pfv_scene_score_q8(e->sc_host.data()) >= e->sc_threshold && e->since_iframe + 1 >= std::max(1, e->sc_min_interval);   // d of pfv_scene_plan: this frame counted
    }
    if (e->n_written == 0 || e->poisoned || (e->gop_max > 0 && e->since_iframe >= e->gop_max)) {   // 1: a forced i-frame
        rc = write_iframe(e, y, u, v);
    } else if (cut) {                                                                               // 1b: a scene cut: an i-frame, no p-frame sizing
        rc = write_iframe(e, y, u, v);
    } else if (!enc_fourstep(s)) {                                                                  // PFV_SEARCH_FULL / _HIER under scene-cut detection: a p-frame at the current rung
        type = 2;
        rc = write_pframe(e, y, u, v, true);
    } else {
        uint32_t psize[kMaxRungs], isize[kMaxRungs], counts[kMaxRungs][kPProbeStats];
        uint64_t psse[kMaxRungs][3], isse[kMaxRungs][3];
        int64_t pq[kMaxRungs][3], iq[kMaxRungs][3];
        const bool rd = pframe_floor(e);
        const bool p_ssim = rd && e->sfloor_p > 0.0, i_ssim = rd && (p_ssim || (e->sfloor_i > 0.0 && s->n_rungs > 1));   // which probe measures each candidate
        if ((rc = probe_pframe_planes(e, y, u, v, psize, &counts[0][0], rd ? &psse[0][0] : nullptr, p_ssim ? &pq[0][0] : nullptr))) return rc;   // 2: one upload, the p-frame sized (and measured) at every rung
        const int rp = p_ssim ? ssim_floor_rung(e, psize, &psse[0][0], &pq[0][0], e->budget_p, e->floor_p, e->sfloor_p)
                     : rd ? floor_rung(e, psize, &psse[0][0], e->budget_p, e->floor_p) : hard_pframe_budget(e) ? budget_rung(s, psize, e->budget_p) : s->rung;
        if (counts[rp][kPProbeCodedAt] == 0 && counts[rp][kPProbeMovedAt] == 0) {                   // 3: nothing to code, nothing moved: a drop frame
            type = 3;
            write_dropframe(e);
        } else if (rd) {                                                                            // 4 under the p-frame floor: the better of p at rp and i at ri
            if ((rc = i_ssim ? ssim_probe_staged(s, false, isize, &isse[0][0], &iq[0][0]) : rd_probe_staged(s, isize, &isse[0][0]))) return rc;
            const int ri = !iframe_rung_rule(e) ? s->rung
                         : e->sfloor_i > 0.0 ? ssim_floor_rung(e, isize, &isse[0][0], &iq[0][0], e->budget_i, e->floor_i, e->sfloor_i)
                         : e->floor_i > 0.0 ? floor_rung(e, isize, &isse[0][0], e->budget_i, e->floor_i) : budget_rung(s, isize, e->budget_i);
            if (rd_prefers_iframe(e, psize[rp], psse[rp], isize[ri], isse[ri], p_ssim ? pq[rp] : nullptr, p_ssim ? iq[ri] : nullptr)) {
                s->rung = ri;
                rc = write_iframe(e, y, u, v, true, nullptr, true);
            } else {                                                                                // 5: a p-frame at rp
                type = 2;
                s->rung = rp;
                rc = write_pframe(e, y, u, v, true);
            }
        } else {
            if ((rc = probe_staged(s, isize))) return rc;                                          // 4: an i-frame that is not larger at rp
            // psize[rp] marked not encodable (0xffffffff) compares as larger than any i-frame that is encodable: the i-frame is taken
            if (isize[rp] != kEntErrOversize && isize[rp] <= psize[rp]) {
                rc = write_iframe(e, y, u, v, true, isize);
            } else {                                                                                // 5: a p-frame at rp
                type = 2;
                s->rung = rp;
                rc = write_pframe(e, y, u, v, true);
            }
        }
    }
    if (!rc && type_out) *type_out = type;
    return rc;
}
// Encoder::encode_dropframe (src/enc.rs:175-180): an i-frame packet with an empty payload
PFV_API int pfv_encoder_encode_dropframe(pfv_encoder *e)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->report_on) e->report_state = -1;
    if (e->ssim_on) e->ssim_state = -1;
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:176)");
    write_dropframe(e);
    return PFV_OK;
}
// Encoder::finish (src/enc.rs:182-188): EOF packet
PFV_API int pfv_encoder_finish(pfv_encoder *e)
{
    if (!e) return fail(nullptr, PFV_ERR_BAD_ARG, "null encoder");
    if (e->finished) return fail(e->ctx, PFV_ERR_STATE, "encoder already finished (src/enc.rs:183)");
    e->finished = true;
    put_packet(e->out, 0, nullptr, 0);
    return PFV_OK;
}
PFV_API int pfv_encoder_bytes(pfv_encoder *e, const uint8_t **data, size_t *len)
{
    if (!e || !data || !len) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_encoder_bytes: bad argument");
    *data = e->out.data();
    *len = e->out.size();
    return PFV_OK;
}
// The reference streams every packet to its writer and keeps nothing (src/enc.rs:190-235); so does this: the bytes produced
// since the last drain are handed over and forgotten, only the current packet is ever resident.
PFV_API int pfv_encoder_drain(pfv_encoder *e, const uint8_t **data, size_t *len)
{
    if (!e || !data || !len) return fail(e ? e->ctx : nullptr, PFV_ERR_BAD_ARG, "pfv_encoder_drain: bad argument");
    e->drained.swap(e->out);
    e->out.clear();
    *data = e->drained.data();
    *len = e->drained.size();
    return PFV_OK;
}
// Drop for Encoder (src/enc.rs:28-34): finishes the stream if the caller did not
PFV_API void pfv_encoder_destroy(pfv_encoder *e)
{
    if (!e) return;
    if (e->rgb_scratch || e->scaler || e->dn || e->sc) {
        (void)hipSetDevice(e->ctx->device);
        (void)hipStreamSynchronize(e->ctx->stream);
        if (e->rgb_scratch) (void)hipFree(e->rgb_scratch);
        if (e->scale_src) (void)hipFree(e->scale_src);
        if (e->dn_src) (void)hipFree(e->dn_src);
        pfv_scaler_destroy(e->scaler);
        pfv_denoiser_destroy(e->dn);
        pfv_scene_detector_destroy(e->sc);
        if (e->sc_dev) (void)hipFree(e->sc_dev);
    }
    pfv_enc_session_destroy(e->hot);
    delete e;
}
