/*
 * pfv_hip_ext.h -- everything of libpfv_hip.so's C ABI that is NOT the drop-in boundary (that is pfv_hip_core.h, included here).
 * Same conventions; `*_dev` entry points take DEVICE pointers and are asynchronous on the context's HIP stream.
 *
 *   [B] THROUGHPUT FORMS of the core's operations -- same bytes, frames and per-call results, another launch shape or residence;
 *       each is parity-tested against the core and the oracle: the *_dev entry points and device memory helpers, HIP graphs, the
 *       session window / frame stride (GOP batching), the device entropy stage of the encoder session (pfv_enc_entropy_*,
 *       pfv_enc_pack_*), sparse pairs and coefficient lists into the decoder session, the batch objects (pfv_batch_*), the GOP-batched
 *       objects (pfv_gop_*), frames left in / taken from device memory, look-ahead threads of pfv_decoder, plane helpers on device planes
 *       (blit, reduce, double, RGB <-> YUV).
 *   [C] DIAGNOSTICS, MEASUREMENT AND TEST HOOKS -- not needed by a caller of the codec and free to change: context options
 *       (pfv_ctx_set_option), events, the synthetic workload generator, the payload serialisers / parsers on their own, object
 *       statistics, and the multi-GPU control plane (pfv_comm_*), which serves bench.py's sharded job, not the codec.
 */
#ifndef PFV_HIP_EXT_H
#define PFV_HIP_EXT_H

#include "pfv_hip_core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same with a priority for the context's HIP stream: > 0 the device's greatest, < 0 its least, 0 the default.  When an
 * encoder and a decoder work side by side on two contexts (a transcoder; bench.py's single-stream schedule), the encoder's launches
 * are the critical path and the decoder's fill the gaps: encoder context high, decoder context low. */
PFV_API int pfv_ctx_create_prio(int device, int priority, pfv_ctx **out);
/* PCI address "domain:bus:device.function" of the context's device (len >= 16): which physical GPU a rank sits on */
PFV_API int pfv_ctx_pci_bus_id(pfv_ctx *ctx, char *out, int len);
/* hipDeviceSynchronize on the context's device (all streams) */
PFV_API int pfv_device_sync(pfv_ctx *ctx);
/* hipStream_t of the context (for callers that enqueue their own work / HIP events) */
PFV_API void *pfv_ctx_stream(pfv_ctx *ctx);

/* [C] Context options (diagnostics / test parametrisation; the defaults are what production wants).  An option applies to the
 * plane-level operators called on the context and to sessions CREATED afterwards (a session keeps the values it was created
 * with).  Results are the same bytes under every value.
 *   PFV_OPT_ENC_TRANSFORM  how the encode kernels evaluate the transforms of the closed loop (src/dct.rs:176-293):
 *       PFV_ENC_TRANSFORM_AUTO (default)  in f32 where that is provably the same arithmetic -- every intermediate an integer
 *                                          below 2^24 for the session's tables, checked at session creation; always true for
 *                                          quality 0..10 -- and in i32 otherwise
 *       PFV_ENC_TRANSFORM_INT             always the i32 kernels
 *   PFV_OPT_DEC_TRANSFORM  how the decode kernels evaluate the inverse transform (src/dct.rs:241-293):
 *       PFV_DEC_TRANSFORM_AUTO (default)  in f32 for every wavefront and pass whose dequantised values v = coefficient x table entry --
 *                                          formed in i32 as ever, wrapped where the reference wraps -- all satisfy |v| <= pfv_dec_float_guard(),
 *                                          the bound below which f32 reproduces the integer butterflies bit for bit; in i32 for the others.
 *                                          Decided on the device from the data: any coefficients, any tables
 *       PFV_DEC_TRANSFORM_INT             always the i32 kernels
 *   PFV_OPT_TILE_COMPACTION  1 (default): the p-frame encoder transforms only CODED macroblocks where that saves work -- a
 *       skipped macroblock is not transformed by the reference either (src/common.rs:221-222) -- by moving the coded macroblocks of
 *       a 128 x 64 tile together before the transform phase; 0: every wavefront transforms its own strip (measurements);
 *       2: the p-frame encoder as TWO kernels (measurements: 17 % slower, profiles/r06_enc_pframe_split.md) -- k_pf_search (search, skip
 *       decision, skipped macroblocks finished) and k_pf_transform (coded macroblocks only, numbered per 64 macroblocks); launches of
 *       the 8-lanes-per-macroblock mapping only, the small-grid mapping ignores it
 *   PFV_OPT_LANE_MAPPING  how the four codec kernels spread a macroblock over lanes:
 *       PFV_LANES_AUTO (default)   by grid size: 8 lanes per macroblock (a wavefront = a strip of 8 macroblocks) for launches that
 *                                  fill the device, 16 (a wavefront = 4 macroblocks, half as long) for launches of fewer than
 *                                  4 096 strips -- one or two 1080p streams per launch, the reference's own usage
 *                                  (src/enc.rs:125-173)
 *       PFV_LANES_PER_MB_8 / PFV_LANES_PER_MB_16   force one of them
 *   PFV_OPT_ENTROPY_DECODE  where pfv_gop_decoder turns packet payloads into coefficients (src/dec.rs:258-296, 378-417):
 *       PFV_ENTROPY_DECODE_AUTO (default)  on the device (k_entd_*: self-synchronising parallel read of the run streams) when the
 *                                          batch's coefficient lists fit the device's free memory, on the host otherwise
 *       PFV_ENTROPY_DECODE_HOST            the host parser pool (n_threads of pfv_gop_decoder_create)
 *       PFV_ENTROPY_DECODE_DEVICE          the device, or PFV_ERR_NOMEM from pfv_gop_decoder_create
 *     Either way a payload the device stage is not sure about (damaged, degenerate code table, periodic content whose read does
 *     not settle) is parsed by the host code, which alone decides about errors.
 *   PFV_OPT_ENTDEC_LANE_BITS / _LAUNCHES / _INNER_ROUNDS  shape of the device stage (measurements, and tests that force the "not settled"
 *       road): payload bits per lane (a multiple of 32 in 32..256, default 256), read launches before the verifying one (1..64, default 3:
 *       the full read k_entd_sync, then k_entd_fix for the seams between its workgroups), settling rounds inside a workgroup of the full
 *       read (1..1024, default 96; a round in which no lane has a new start ends them) */
typedef enum pfv_option {
    PFV_OPT_ENC_TRANSFORM = 1, PFV_OPT_TILE_COMPACTION = 2, PFV_OPT_LANE_MAPPING = 3, PFV_OPT_ENTROPY_DECODE = 4,
    PFV_OPT_ENTDEC_LANE_BITS = 5, PFV_OPT_ENTDEC_LAUNCHES = 6, PFV_OPT_ENTDEC_INNER_ROUNDS = 7, PFV_OPT_DEC_TRANSFORM = 8
} pfv_option;
enum { PFV_ENTROPY_DECODE_AUTO = 0, PFV_ENTROPY_DECODE_HOST = 1, PFV_ENTROPY_DECODE_DEVICE = 2 };
enum { PFV_LANES_AUTO = 0, PFV_LANES_PER_MB_8 = 1, PFV_LANES_PER_MB_16 = 2 };
enum { PFV_ENC_TRANSFORM_AUTO = 0, PFV_ENC_TRANSFORM_INT = 1 };
enum { PFV_DEC_TRANSFORM_AUTO = 0, PFV_DEC_TRANSFORM_INT = 1 };
PFV_API int pfv_ctx_set_option(pfv_ctx *ctx, int option, int value);
PFV_API int pfv_ctx_get_option(pfv_ctx *ctx, int option, int *value);

/* [C] Timing events on the context's stream (HIP events): record costs a microsecond or two, so every launch of a pass can be
 * bracketed without disturbing it; pfv_event_elapsed_ms waits for the later event. */
typedef struct pfv_event pfv_event;
PFV_API int pfv_event_create(pfv_ctx *ctx, pfv_event **out);
PFV_API int pfv_event_record(pfv_event *e);
PFV_API int pfv_event_elapsed_ms(pfv_event *start, pfv_event *stop, float *ms);
PFV_API void pfv_event_destroy(pfv_event *e);
/* [B] Ordering between contexts (each has its own HIP stream): ctx's stream waits, on the device, for an event recorded on another
 * context's stream.  This is how a decoder on one context consumes what an encoder on another produces while the encoder is
 * already working on the next frame -- Encoder and Decoder are independent objects in the reference (src/enc.rs:12-26,
 * src/dec.rs:15-28), and for a single stream the device is far from full with one of them. */
PFV_API int pfv_ctx_wait_event(pfv_ctx *ctx, pfv_event *e);

/* [B] HIP graphs over the `*_dev` entry points.  The reference's caller is one Encoder per stream, one call per frame
 * (src/enc.rs:125-173); for a single stream the launches, not the kernels, are the cost.  Every `*_dev` call made between
 * pfv_graph_begin and pfv_graph_end on this context is recorded instead of executed (stream capture); pfv_graph_launch
 * replays the whole sequence -- e.g. the 30 launches of a GOP-15 encode + decode -- as one launch.  Device pointers are baked
 * into the graph.  The recorded sequence must start with an i-frame step of every session it touches (an i-frame reads no
 * previous state, src/enc.rs:84-97), or contain an even number of frame steps per session, so that the sessions' ping-pong
 * state after a replay equals the state after the recording.  Host-pointer entry points cannot be recorded. */
typedef struct pfv_graph pfv_graph;
PFV_API int pfv_graph_begin(pfv_ctx *ctx);
PFV_API int pfv_graph_end(pfv_ctx *ctx, pfv_graph **out);
PFV_API int pfv_graph_launch(pfv_graph *g);
PFV_API void pfv_graph_destroy(pfv_graph *g);

/* VideoPlane::blit (src/plane.rs:20-29) on device-resident planes. */
PFV_API int pfv_blit_dev(pfv_ctx *ctx, uint8_t *dst, int dst_w, int dst_h, const uint8_t *src, int src_w, int src_h,
                         int dx, int dy, int sx, int sy, int sw, int sh);

/* VideoPlane::reduce (src/common.rs:523-536, point-sampled 2x decimation, dst = src_w/2 x src_h/2) and
 * VideoPlane::double (:538-556, nearest 2x upsampling, dst = 2 src_w x 2 src_h) on device-resident planes. */
PFV_API int pfv_reduce_dev(pfv_ctx *ctx, uint8_t *dst, const uint8_t *src, int src_w, int src_h);
PFV_API int pfv_double_dev(pfv_ctx *ctx, uint8_t *dst, const uint8_t *src, int src_w, int src_h);
/* The RGB <-> YCbCr helpers of the reference's tests (src/lib.rs:337-394; JPEG-conversion matrix in f32, `as u8`):
 * interleaved RGB8 (width*height*3) -> packed Y|U|V 4:2:0 frame as load_frame + VideoFrame::from_planes produce it
 * (chroma point-sampled at even pixels, src/frame.rs:51-59), and back as save_frame does (chroma doubled,
 * src/common.rs:538-556).  width, height even.  Device-resident buffers. */
PFV_API int pfv_rgb_to_yuv420_dev(pfv_ctx *ctx, const uint8_t *rgb_dev, int width, int height, uint8_t *frame_dev);
PFV_API int pfv_yuv420_to_rgb_dev(pfv_ctx *ctx, const uint8_t *frame_dev, int width, int height, uint8_t *rgb_dev);

/* ------------------------------------------------------------------ multi-GPU control plane (one process per GPU, RCCL over xGMI)  [C]
 * The path shards by stream and by GOP (src/enc.rs:12-26, 84-97): no data-path collective exists.  These carry the few hundred
 * bytes that do travel -- the assignment table (broadcast) and the per-rank counters (reduction / gather) -- on the context's
 * HIP stream.  Rank 0 creates the id, every rank of the job gets the same 128 bytes over the launcher's own channel
 * (pretty-fast-video_amd/comm.py: TCP on MASTER_ADDR) and calls pfv_comm_init on the context of ITS device.  librccl.so is
 * opened at run time; PFV_ERR_NO_DEVICE when it is missing.  world = 1 is legal (a 1-rank communicator).  A communicator
 * belongs to its context (it enqueues on the context's stream): destroy it first, or leave it to pfv_ctx_destroy, which tears down
 * the communicators still alive.  PFV_ERR_STATE while the context records a graph (pfv_graph_begin). */
typedef struct pfv_comm pfv_comm;
enum { PFV_COMM_SUM = 0, PFV_COMM_MAX = 1 };
PFV_API int pfv_comm_unique_id(uint8_t id_out[128]);
PFV_API int pfv_comm_init(pfv_ctx *ctx, int rank, int world, const uint8_t id[128], pfv_comm **out);
PFV_API int pfv_comm_rank(const pfv_comm *c);
PFV_API int pfv_comm_world(const pfv_comm *c);
/* in-place collectives on DEVICE buffers, asynchronous on the context's stream */
PFV_API int pfv_comm_broadcast_dev(pfv_comm *c, void *buf_dev, size_t bytes, int root);
PFV_API int pfv_comm_allreduce_f64_dev(pfv_comm *c, double *buf_dev, size_t count, int op);
PFV_API int pfv_comm_allgather_dev(pfv_comm *c, const void *send_dev, void *recv_dev, size_t bytes_per_rank);
/* host values (count <= 64): staged through the device, reduced on the stream, synchronised */
PFV_API int pfv_comm_allreduce_f64(pfv_comm *c, double *values, size_t count, int op);
/* all ranks have arrived and everything enqueued before on their streams is done */
PFV_API int pfv_comm_barrier(pfv_comm *c);
/* a communicator belongs to its context: pfv_ctx_destroy tears down the ones still alive, and their handles are invalid from then on */
PFV_API void pfv_comm_destroy(pfv_comm *c);

/* ------------------------------------------------------------------ synthetic workload (not a reference interface)  [C]
 * The reference's fixtures are Git-LFS stubs; tests and benchmarks run on an integer-only synthetic video (SURVEY.md
 * section 8d) that is generated where it is consumed: frame `t` of n_streams streams (stream s seeded with seeds[s], a HOST
 * array) as packed Y|U|V frames back to back in frames_dev.  Byte-identical to synth.SyntheticStream(w, h, seed).frame(t). */
PFV_API int pfv_synth_frames_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint64_t *seeds, int t,
                                 uint8_t *frames_dev);
/* The same with the content kind chosen: PFV_SYNTH_PAN (what pfv_synth_frames_dev generates: the whole texture pans, noise on
 * half the macroblocks: ~85 % of a quality-5 p-frame is coded) or PFV_SYNTH_LOW_MOTION (static background, four noisy rectangles
 * of about a quarter of the frame's width and height moving over it: ~25 % coded, the rest skipped, src/common.rs:221-222).
 * PFV_SYNTH_STATIC: the background alone (every p-frame macroblock skipped: the floor of the p-frame encoder, its search).
 * Byte-identical to synth.SyntheticStream(w, h, seed, kind).frame(t). */
enum { PFV_SYNTH_PAN = 0, PFV_SYNTH_LOW_MOTION = 1, PFV_SYNTH_STATIC = 2 };
PFV_API int pfv_synth_frames_kind_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint64_t *seeds, int t, int kind,
                                      uint8_t *frames_dev);

/* ------------------------------------------------------------------ device memory helpers  [B] */
PFV_API int pfv_dev_alloc(pfv_ctx *ctx, size_t bytes, void **out);
PFV_API int pfv_dev_free(pfv_ctx *ctx, void *p);
/* device-to-device copy, asynchronous on the context's stream (ordered like every *_dev call) */
PFV_API int pfv_dev_copy(pfv_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
/* page-locked host memory (hipHostMalloc) for the buffers handed to the host-pointer entry points: uploads / downloads
 * from it run at PCIe rate instead of bouncing through the runtime's staging (the reference's Vec<u8> planes,
 * src/plane.rs:1-5, would be allocated here by a binding that cares) */
PFV_API int pfv_host_alloc(pfv_ctx *ctx, size_t bytes, void **out);
PFV_API int pfv_host_free(pfv_ctx *ctx, void *p);
PFV_API int pfv_dev_upload(pfv_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
PFV_API int pfv_dev_download(pfv_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* Encoder::encode_iframe, hot-path part (src/enc.rs:84-97): per plane encode_plane ->
 * decode_plane -> prev_frame.blit, fused into one launch over all streams and planes. */
PFV_API int pfv_enc_iframe_dev(pfv_enc_session *s, const uint8_t *frames_dev, int16_t *coef_dev);
/* Encoder::encode_pframe, hot-path part (src/enc.rs:134-147). */
PFV_API int pfv_enc_pframe_dev(pfv_enc_session *s, const uint8_t *frames_dev, int8_t *mv_dev, uint8_t *has_coef_dev,
                               int16_t *coef_dev);
/* GOP-batched use of a session.  The n_streams slots of a session need not be different videos: encode_iframe never reads
 * prev_frame and overwrites every plane of it (src/enc.rs:84-97), so the GOPs of ONE stream are independent of each other and
 * can occupy the slots -- frame t of every GOP in one launch (bench.py --workload config5; pfv_gop_encoder below).
 *   pfv_enc_session_set_frame_stride: bytes between the input frames of consecutive slots (0 = packed, the default).  With
 *       the stream's frames resident in display order and equal GOPs of G frames, stride = G * pfv_frame_bytes and
 *       frames_dev = first frame + t * pfv_frame_bytes make slot g read frame g * G + t.
 *   pfv_enc_session_set_window: the following pfv_enc_*frame_dev / pfv_enc_pack_*_dev calls work on slots
 *       [first, first + count) only (a shorter last GOP); the buffers keep their full-width layout, entries of other slots are
 *       left alone.  A slot left out of a frame step keeps no usable prev_frame: its next frame must be an i-frame.
 * The host-buffer entry points need the full window and packed frames (PFV_ERR_STATE otherwise). */
PFV_API int pfv_enc_session_set_frame_stride(pfv_enc_session *s, size_t stride_bytes);
PFV_API int pfv_enc_session_set_window(pfv_enc_session *s, int first, int count);
/* device pointer of stream `stream`'s current prev_frame (padded Y|U|V), for checks */
PFV_API const uint8_t *pfv_enc_prev_frame_dev(pfv_enc_session *s, int stream);

/* ------------------------------------------------------------------ device entropy stage (encoder session)  [B]
 * The reference serialises each frame on one host thread: rle_encode per macroblock (src/rle.rs:9-47), one histogram
 * and Huffman tree per frame (rle.rs:40-66, src/huffman.rs:71-119), LSB-first bit packing into the packet payload
 * (write_iframe_packet src/enc.rs:237-320, write_pframe_packet :332-470).  These entry points build the same payload
 * bytes on the device from the buffers pfv_enc_iframe_dev / pfv_enc_pframe_dev produced, so only the compressed
 * payload crosses PCIe.  Payloads are byte-identical to pfv_serialize_iframe_payload / pfv_serialize_pframe_payload. */
/* upper bound of a payload for this geometry, in bytes (multiple of 4) */
PFV_API size_t pfv_payload_worst_case(int width, int height);
/* allocates the stage's buffers; payload_cap = bytes per stream (0: pfv_payload_worst_case).  Idempotent. */
PFV_API int pfv_enc_entropy_enable(pfv_enc_session *s, size_t payload_cap);
/* 1: the stage runs on its own HIP stream, so the (memory-bound) entropy kernels of frame t overlap the (VALU-bound)
 * encode kernel of frame t+1.  The caller must then alternate between TWO sets of device buffers for the encode outputs
 * it packs.  pfv_enc_payload_sizes / _fetch synchronise with the stage; pfv_enc_entropy_join makes the context's stream
 * wait for it without blocking the host.  0 (default): everything on the context's stream. */
PFV_API int pfv_enc_entropy_set_async(pfv_enc_session *s, int on);
PFV_API int pfv_enc_entropy_join(pfv_enc_session *s);
/* coef_dev / mv_dev / has_coef_dev: device buffers in the layout the encode entry points write (n_streams wide) */
PFV_API int pfv_enc_pack_iframe_dev(pfv_enc_session *s, const int16_t *coef_dev);
PFV_API int pfv_enc_pack_pframe_dev(pfv_enc_session *s, const int8_t *mv_dev, const uint8_t *has_coef_dev,
                                    const int16_t *coef_dev);
/* byte count of each stream's payload from the last pack call (synchronises).  PFV_ERR_FORMAT: a coefficient needs more
 * than 15 size bits (the reference panics, rle.rs:44); PFV_ERR_NOMEM: a payload exceeds the capacity.  sizes_out is
 * filled either way (0 for failed streams). */
PFV_API int pfv_enc_payload_sizes(pfv_enc_session *s, uint32_t *sizes_out);
/* every stream's payload with one device-to-host copy: gathered back to back on the device (16-byte aligned starts) into
 * `out` (cap bytes, ideally from pfv_host_alloc); stream s occupies out[offsets_out[s] .. + sizes_out[s]).  Synchronises;
 * errors as pfv_enc_payload_sizes, PFV_ERR_NOMEM when cap is too small. */
PFV_API int pfv_enc_payloads_fetch(pfv_enc_session *s, uint8_t *out, size_t cap, uint32_t *sizes_out, uint64_t *offsets_out);
PFV_API const uint8_t *pfv_enc_payload_dev(pfv_enc_session *s, int stream);
PFV_API size_t pfv_enc_payload_capacity(pfv_enc_session *s);
/* first nbytes of one stream's payload to the host (synchronises) */
PFV_API int pfv_enc_payload_fetch(pfv_enc_session *s, int stream, uint8_t *out_host, size_t nbytes);
/* Decoder::decode_iframe after entropy decoding (src/dec.rs:298-323 -> deserialize_plane
 * :450-479 -> decode_plane_into).  qidx: the three per-plane q-table indices of the
 * packet (src/dec.rs:249-251). */
PFV_API int pfv_dec_iframe_dev(pfv_dec_session *s, const int16_t *coef_dev, const uint8_t qidx[3]);
/* Decoder::decode_pframe after entropy decoding (src/dec.rs:419-445 -> :481-517). */
PFV_API int pfv_dec_pframe_dev(pfv_dec_session *s, const int8_t *mv_dev, const uint8_t *has_coef_dev,
                               const int16_t *coef_dev, const uint8_t qidx[3]);
/* Sparse forms: the non-zero coefficients as n (flat index into [stream][macroblock][256], value) pairs -- what the
 * bit parser (src/dec.rs:261-296, 378-417) produces before it is spread into the dense vector; ~10x fewer bytes over
 * PCIe.  Same result as the dense call on the expanded array; indices past the frame are ignored. */
PFV_API int pfv_dec_iframe_sparse(pfv_dec_session *s, const uint32_t *idx, const int16_t *val, size_t n, const uint8_t qidx[3]);
PFV_API int pfv_dec_pframe_sparse(pfv_dec_session *s, const int8_t *mv, const uint8_t *has_coef, const uint32_t *idx,
                                  const int16_t *val, size_t n, const uint8_t qidx[3]);
/* Coefficient lists (round 5): a frame's non-zero coefficients as 32-bit entries instead of its dense [macroblock][256] array -- the form the
 * stream decoders' entropy stage hands to the decode kernels, which expand a strip's entries straight into their LDS zigzag stage (the
 * reference expands runs into the macroblock it is about to decode, src/dec.rs:258-296, 378-417); nothing is cleared and nothing but the
 * values travels.
 *   entry   value (i16) << 16 | (macroblock index & 255) << 8 | position in the macroblock (0..255), ascending by (macroblock, position);
 *   count   per macroblock m and one more behind the last (total_blocks + 1 per frame): the entries that belong to macroblocks before m,
 *           so m owns [count[m], count[m + 1]); a macroblock a p-frame skips owns none.  The counts are the kernels' loop bounds: they
 *           are not validated on the device.
 * entries_dev: per slot of the session's window a DEVICE pointer to the slot's list (a device array of device pointers);
 * counts_dev: [slot][total_blocks + 1].  Same result as the dense call on the expanded arrays. */
PFV_API int pfv_dec_iframe_lists_dev(pfv_dec_session *s, const uint32_t *const *entries_dev, const uint32_t *counts_dev, const uint8_t qidx[3]);
PFV_API int pfv_dec_pframe_lists_dev(pfv_dec_session *s, const int8_t *mv_dev, const uint8_t *has_coef_dev, const uint32_t *const *entries_dev,
                                     const uint32_t *counts_dev, const uint8_t qidx[3]);
/* host helper: one frame's dense coefficients ([total_blocks][256]; has_coef NULL: every macroblock is read) as a coefficient list.  Room for
 * `cap` entries and total_blocks + 1 counts; *n_out = entries written; returns 1 when `cap` does not suffice (total_blocks x 256 always does). */
PFV_API int pfv_coef_lists_from_dense(const int16_t *coef, const uint8_t *has_coef, int total_blocks, uint32_t *entries_out, size_t cap,
                                      uint32_t *counts_out, size_t *n_out);
/* Decoder::advance_frame's crop of framebuffer into retframe (src/dec.rs:195-197,
 * 209-211): frames_out = n_streams unpadded frames (Y|U|V). */
PFV_API int pfv_dec_get_frame_dev(pfv_dec_session *s, uint8_t *frames_out_dev);
/* Fused form of the same crop: once a device buffer of n_streams unpadded frames is set, every
 * following pfv_dec_iframe_dev / pfv_dec_pframe_dev also writes the retframe into it (the decode
 * kernels store each reconstructed row twice: padded framebuffer + cropped retframe), saving the
 * separate blit pass.  NULL switches it off. */
PFV_API int pfv_dec_set_output_dev(pfv_dec_session *s, uint8_t *frames_out_dev);
/* The same with `stride_bytes` (>= pfv_frame_bytes; 0 = packed) between the retframes of consecutive slots, and the slot window
 * of the *_dev calls -- the decoder-side halves of the GOP-batched use described at pfv_enc_session_set_window
 * (decode_plane_into overwrites the whole framebuffer, src/common.rs:477-496): with stride = G * pfv_frame_bytes and
 * frames_out_dev = first frame + t * pfv_frame_bytes the decoded stream appears in display order. */
PFV_API int pfv_dec_set_output_strided_dev(pfv_dec_session *s, uint8_t *frames_out_dev, size_t stride_bytes);
PFV_API int pfv_dec_session_set_window(pfv_dec_session *s, int first, int count);
/* [C] The bound of PFV_DEC_TRANSFORM_AUTO, and which road a session's launches took (tests, measurements).  A wavefront is one launch's
 * unit of work that owns a macroblock: a strip of 8 macroblocks, or 4 under the 16-lane mapping.  enable_path_stats(on = 1) starts
 * counting from zero (again), 0 stops; path_stats waits for the stream and reports, since then, the wavefronts that ran a pass of the
 * inverse transform in i32 because the guard failed, and all wavefronts launched (p-frame wavefronts without a coded macroblock included:
 * they transform nothing).  A session that does not count hands its kernels a null counter. */
PFV_API int pfv_dec_float_guard(void);
PFV_API int pfv_dec_session_enable_path_stats(pfv_dec_session *s, int on);
PFV_API int pfv_dec_session_path_stats(pfv_dec_session *s, int64_t *int_waves, int64_t *total_waves);
/* 1 (default): packet payloads come from the device entropy stage; 0: from the host serialisers.  Same bytes. */
PFV_API int pfv_encoder_set_device_entropy(pfv_encoder *e, int on);
/* ------------------------------------------------------------------ distortion on the device  [B]
 * How far two frames are apart, measured where they lie: the sum of squared differences per plane and per macroblock, and PSNR from it.
 * The reference's only rate / quality control is `quality` 0..10 (src/enc.rs:37-51); these say what a setting costs in fidelity without
 * a frame leaving HBM.  Only pixels inside the picture count (the plane's w x h): padding of a padded operand and the part of an edge
 * macroblock beyond the picture add nothing.  Integer arithmetic, exact; no atomics and nothing to clear, so a call is two kernel nodes of a
 * recorded graph.  Each operand is a PACKED frame (pfv_frame_bytes, plane stride = plane width) or a PADDED one (pfv_padded_frame_bytes,
 * plane stride = pfv_pad16(width): prev_frame / the framebuffer), with its own byte stride between streams; a and b may be the same buffer.
 *   sse_dev     uint64_t[n_streams][3] (Y, U, V)
 *   mb_sse_dev  uint32_t[n_streams][pfv_total_blocks], macroblocks in frame order (Y, U, V; raster inside a plane: the index space of mv /
 *               has_coef), or NULL: the map then goes to scratch of the context / session.  That scratch is allocated by the first call that
 *               needs it; while the context records a graph such a call returns PFV_ERR_STATE (pass a map buffer, or call once before). */
enum { PFV_FRAME_PACKED = 0, PFV_FRAME_PADDED = 1 };
/* stride 0 = frames back to back in the operand's layout.  Asynchronous on the context's stream. */
PFV_API int pfv_frames_sse_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a_dev, int a_layout, size_t a_stride,
                               const uint8_t *b_dev, int b_layout, size_t b_stride, uint64_t *sse_dev, uint32_t *mb_sse_dev);
/* host buffers, both PACKED; mb_sse_out may be NULL; synchronises */
PFV_API int pfv_frames_sse(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a, const uint8_t *b, uint64_t *sse_out,
                           uint32_t *mb_sse_out);
/* 10 * log10(255^2 * n_samples / sse) in double; +INFINITY when sse == 0; NaN when n_samples == 0 */
PFV_API double pfv_psnr(uint64_t sse, uint64_t n_samples);
/* the frames just handed to pfv_enc_iframe_dev / pfv_enc_pframe_dev against the session's CURRENT prev_frame (= what a decoder will show
 * for them).  Honours the session's window and frame stride; the outputs keep the full-width [n_streams] layout, entries of slots outside
 * the window are left alone. */
PFV_API int pfv_enc_distortion_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint64_t *sse_dev, uint32_t *mb_sse_dev);
/* packed frames against the decoder session's current framebuffer, same conventions: the session's window, and its output stride
 * (pfv_dec_set_output_strided_dev; 0 = back to back) as the stride between the frames of consecutive slots */
PFV_API int pfv_dec_distortion_dev(pfv_dec_session *s, const uint8_t *frames_dev, uint64_t *sse_dev, uint32_t *mb_sse_dev);
/* pfv_encoder: what the last encode_* call wrote and how far its reconstruction is from the frame it was given.  With reports on, one
 * more small launch follows the encode kernel and 24 bytes come back with the payload size (or with the host path's downloads); the
 * stream bytes are the same.  pfv_gop_encoder and pfv_batch_encoder have no reports: their batches are collected late and a batch that
 * outgrows its arena is encoded again. */
typedef struct pfv_frame_report {
    int32_t  type;          /* 1 i-frame, 2 p-frame, 3 drop frame */
    uint32_t packet_bytes;  /* 5-byte packet header + payload, as written to the stream */
    uint64_t sse[3];        /* Y,U,V; zeros for a drop frame */
    double   psnr[3];       /* pfv_psnr per plane */
    double   psnr_yuv;      /* pfv_psnr(sse[0]+sse[1]+sse[2], all samples of the frame) */
} pfv_frame_report;
PFV_API int pfv_encoder_set_frame_report(pfv_encoder *e, int on);               /* default 0 */
/* of the last encode_* call; PFV_ERR_STATE when reports are off, no frame has been encoded, or that call failed */
PFV_API int pfv_encoder_frame_report(pfv_encoder *e, pfv_frame_report *out);

/* ------------------------------------------------------------------ structural similarity on the device  [B]
 * Squared error rates the blocking of a coarse rung far too kindly; this is the structural similarity index (SSIM) in the integer form the
 * common video tools use -- 8 x 8 windows at stride 4, so windows straddle the edges of the 8 x 8 transform blocks -- measured where the
 * frames lie.  Operands, layouts, strides and the scratch rule are those of pfv_frames_sse_dev.  Per plane (w x h, 8-bit), on its own:
 *   blocks    bw = w >> 2, bh = h >> 2 blocks of 4 x 4 pixels; pixels beyond 4 bw or 4 bh belong to no block, padding never counts.
 *             Per block, in integers: s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum ab.
 *   windows   one per (bx, by) with bx + 1 < bw and by + 1 < bh: the sums of blocks (bx, by), (bx + 1, by), (bx, by + 1), (bx + 1, by + 1) added
 *             together (64 pixels); max(0, bw - 1) * max(0, bh - 1) per plane (pfv_ssim_windows).
 *   value     c1 = 416, c2 = 235963 ((0.01 * 255)^2 * 64 and (0.03 * 255)^2 * 64 * 63, rounded);
 *                 vars = 64 ss - s1^2 - s2^2       covar = 64 s12 - s1 s2
 *                 n1 = 2 s1 s2 + c1   n2 = 2 covar + c2   d1 = s1^2 + s2^2 + c1   d2 = vars + c2      (exact in int32, all below 2^30)
 *                 ssim = (f32(n1) * f32(n2)) / (f32(d1) * f32(d2))      IEEE single precision, a true division; in [-1, 1]
 *                 q = rint(ssim * 2^24) as int32, round to nearest even
 *   ssim_q24_dev     int64_t[n_streams][3] (Y, U, V): the sum of q over the plane's windows
 *   mb_ssim_q24_dev  int32_t[n_streams][pfv_total_blocks], the index space of mv / has_coef: the sum of q over the windows whose top-left
 *                    pixel lies in the macroblock (at most 16, so |entry| <= 2^28; 0 without windows), or NULL: the map then goes to scratch
 *                    of the context / session under the rule of pfv_frames_sse_dev (PFV_ERR_STATE when that needs an allocation inside a
 *                    graph recording).
 * Every entry of both outputs is written by every call; nothing is accumulated or cleared, and there are no atomics: integer sums do not
 * depend on launch shape or arrival order, so two calls on the same input, and any graph replay, are bit-identical.  Two launches, k_ssim_mb +
 * k_ssim_sum (csrc/pfv_ssim_kernels.hip).  Measured on one MI355X, 96 x 1080p, packed against padded: see profiles/quality_ssim.md. */
PFV_API int pfv_frames_ssim_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a_dev, int a_layout, size_t a_stride,
                                const uint8_t *b_dev, int b_layout, size_t b_stride, int64_t *ssim_q24_dev, int32_t *mb_ssim_q24_dev);
/* host buffers, both PACKED; mb_out may be NULL; synchronises */
PFV_API int pfv_frames_ssim(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *a, const uint8_t *b, int64_t *ssim_q24_out,
                            int32_t *mb_out);
/* windows per plane (Y, U, V) of a width x height frame; PFV_ERR_BAD_ARG for dimensions a frame cannot have */
PFV_API int pfv_ssim_windows(int width, int height, uint32_t out[3]);
/* q24_sum / (2^24 * windows) in double: the mean SSIM of the windows; NaN when windows == 0 */
PFV_API double pfv_ssim(int64_t q24_sum, uint64_t windows);
/* the sessions' own comparisons: operands, window, frame / output stride and slot semantics of pfv_enc_distortion_dev /
 * pfv_dec_distortion_dev; entries of slots outside the window are left alone */
PFV_API int pfv_enc_ssim_dev(pfv_enc_session *s, const uint8_t *frames_dev, int64_t *ssim_q24_dev, int32_t *mb_dev);
PFV_API int pfv_dec_ssim_dev(pfv_dec_session *s, const uint8_t *frames_dev, int64_t *ssim_q24_dev, int32_t *mb_dev);
/* pfv_encoder: the SSIM between the frame the last encode_* call was given and its reconstruction.  A switch of its own, independent of the
 * frame reports: with it on, one more pair of small launches follows the encode kernel and 24 bytes come back with the payload size (or with
 * the host path's downloads); the stream bytes are the same.  pfv_gop_encoder and pfv_batch_encoder have none, for the reason given for
 * the reports. */
typedef struct pfv_frame_ssim {
    int64_t  q24[3];      /* Y,U,V; zeros for a drop frame */
    uint32_t windows[3];
    double   ssim[3];     /* pfv_ssim per plane; 1 for a drop frame */
    double   ssim_all;    /* pfv_ssim(sum of q24, sum of windows); 1 for a drop frame */
} pfv_frame_ssim;
PFV_API int pfv_encoder_set_frame_ssim(pfv_encoder *e, int on);                 /* default 0 */
/* of the last encode_* call; PFV_ERR_STATE when the switch is off, no frame has been encoded, or that call failed */
PFV_API int pfv_encoder_frame_ssim(pfv_encoder *e, pfv_frame_ssim *out);

/* ------------------------------------------------------------------ out-of-loop deblocking  [B]
 * The format has no loop filter: the frames shown are the bare 8 x 8-block reconstruction, and the coarse rungs of a ladder block visibly.
 * This is a POST-filter: it runs on the frame that is displayed and never on the framebuffer the next p-frame predicts from, so streams,
 * decoder state and every parity with the reference stay bit for bit what they are.  Off by default.
 *
 * The filter (normative) works per plane of w x h 8-bit samples, each plane on its own, in integers only.  S is the plane's strength,
 * 0 .. 12.  S = 0 copies the plane.  One edge takes four samples in a line across it, A B | C D; the edge lies between B and C:
 *     tdiv(a, n)  = division truncating toward zero (NOT an arithmetic shift: a may be negative)
 *     d   = tdiv(A - 4B + 4C - D, 8)
 *     d1  = sign(d) * max(0, |d| - max(0, 2 * (|d| - S)))     ramps up to S, back to 0 at 2S: a real edge is left alone
 *     d2  = clamp(tdiv(A - D, 4), -(|d1| >> 1), |d1| >> 1)
 *     B'  = clamp(B + d1, 0, 255)     C' = clamp(C - d1, 0, 255)     A' = A - d2     D' = D + d2
 * A' and D' need no clamp: they move toward each other by at most |A - D| / 4.
 *   Stage 1, vertical edges.    For every row y < h and every x with x % 8 == 0, x >= 8 and x + 1 < w, apply the edge with A,B,C,D = samples
 *                               x-2, x-1, x, x+1 of the input row.
 *   Stage 2, horizontal edges.  For every column x < w and every y with y % 8 == 0, y >= 8 and y + 1 < h, apply the edge to rows y-2, y-1, y,
 *                               y+1 of the STAGE-1 RESULT.
 * Edges within a stage touch disjoint samples (they are 8 apart and each reaches +-2), so each stage is order-free and the result does not
 * depend on the launch shape.  Samples outside w x h never take part -- the padding of a padded operand included.  The grid is the transform
 * grid of each plane: 8 x 8 in luma and in each chroma plane at its own resolution; motion-compensated edges off the grid are not searched
 * for.
 * The automatic strength of a plane comes from its q-table: S = min(12, q[0] >> 1), q[0] being the DC quantiser (index 0 in raster and in
 * zigzag order alike; 0 .. 65535, decoders accept hostile tables).  That is 0 at quality 0 and 1 / 2 / 5 for intra luma at qualities
 * 2 / 5 / 10, and twice that for chroma and for inter tables, whose error is about twice as large.
 * One launch, k_deblock (csrc/pfv_deblock_kernels.hip); no atomics, nothing allocated: a call is one kernel node of a recorded graph.
 * Measured on one MI355X, 96 x 1080p: see profiles/deblock.md. */
PFV_API int pfv_deblock_strength(const int32_t qtable[64]);
/* src: n_streams frames, PACKED or PADDED (pfv_frames_sse_dev), src_stride bytes apart (0 = back to back in its layout); dst: PACKED frames
 * dst_stride bytes apart (0 = back to back).  Every byte of the n_streams pictures is written, no byte between or beyond them.
 * strength: per plane (Y, U, V).  Asynchronous on the context's stream.  PFV_ERR_BAD_ARG for a strength above 12, a null buffer, a
 * destination stride below pfv_frame_bytes, or source and destination ranges that overlap: in-place is not supported. */
PFV_API int pfv_frames_deblock_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src_dev, int src_layout, size_t src_stride,
                                   uint8_t *dst_dev, size_t dst_stride, const uint8_t strength[3]);
/* host buffers, PACKED on both sides; synchronises */
PFV_API int pfv_frames_deblock(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src, uint8_t *dst, const uint8_t strength[3]);
/* A decoder session's switch.  AUTO: per plane, pfv_deblock_strength of the table that the LAST decode call's qidx named (`strength` is
 * ignored, may be NULL; before the first decode call the strengths are 0); FIXED: `strength`.  While on, every way a frame leaves the session is the filtered picture -- pfv_dec_get_frame,
 * pfv_dec_get_frame_dev and the output set by pfv_dec_set_output_dev / _strided_dev -- produced by one k_deblock from the current
 * framebuffer, honouring the window and the output stride; the decode kernels are then launched without their fused crop and k_crop_frames
 * is not launched.  The framebuffer, the ping-pong, pfv_dec_framebuffer, pfv_dec_distortion_dev and pfv_dec_ssim_dev are untouched (the
 * latter two keep comparing against the framebuffer).  With mode OFF every launch is exactly what it is without this switch.
 * pfv_gop_decoder and pfv_batch_decoder drive their sessions' fields directly and stay without the switch. */
enum { PFV_DEBLOCK_OFF = 0, PFV_DEBLOCK_AUTO = 1, PFV_DEBLOCK_FIXED = 2 };
PFV_API int pfv_dec_set_deblock(pfv_dec_session *s, int mode, const uint8_t strength[3]);
/* pfv_decoder: forwards to its session; the callback then receives filtered frames, on the host and on the device output path */
PFV_API int pfv_decoder_set_deblock(pfv_decoder *d, int mode, const uint8_t strength[3]);

/* ------------------------------------------------------------------ RGB / RGBA texture output  [B]
 * The last step of a decoder: the planar Y | U | V 4:2:0 frame as interleaved pixels a renderer can sample (the reference's README wishes for
 * decoding "directly into a game-ready texture").  One launch, k_present_rgb (csrc/pfv_present_kernels.hip), converts n_streams frames; the
 * source is PACKED or PADDED with its own stream stride (pfv_frames_sse_dev), so a session's padded framebuffer is read where it lies.
 *   format          bytes / pixel   byte order
 *   PFV_PIX_RGB8    3               R, G, B
 *   PFV_PIX_RGBA8   4               R, G, B, 255
 *   PFV_PIX_BGRA8   4               B, G, R, 255
 * Arithmetic (normative): the reference's save_frame (src/lib.rs:361-394).  For the pixel (x, y), Y its luma sample and U, V the chroma
 * samples at (x >> 1, y >> 1) (nearest doubling), in IEEE single precision, evaluated left to right, every product and sum rounded on its
 * own (no fused multiply-add):
 *     u = f32(U) - 128     v = f32(V) - 128     yy = f32(Y)
 *     R = yy + 1.402 * v     G = yy - 0.344136 * u - 0.714136 * v     B = yy + 1.772 * u
 * each converted as Rust's `as u8`: truncated toward zero, saturated to 0 .. 255.  These are the expressions of pfv_yuv420_to_rgb_dev.
 * Width and height are positive, even and fit u16.
 * Destination: rows `pitch` bytes apart (0 = pfv_rgb_row_bytes), pictures `stride` bytes apart (0 = pitch x height).  Exactly the
 * width x bytes-per-pixel bytes of every row of every picture are written: nothing in the pitch padding, between or beyond the pictures.
 * Aligned operands (source planes and rows to 4 bytes; destination base, pitch and stride to 4 bytes for RGB8, 16 for the others) take
 * 4-byte loads and 12- / 16-byte non-temporal stores, anything else a byte-granular path with the same result.  No atomics, nothing
 * allocated: a call is one kernel node of a recorded graph.  Measured on one MI355X: see profiles/present.md.
 * PFV_ERR_BAD_ARG: a format or layout that does not exist, a null buffer, dimensions a frame cannot have, a pitch below the row size, a
 * stride below pitch x height, a source stride below its layout's frame size, source and destination ranges that overlap. */
enum { PFV_PIX_RGB8 = 0, PFV_PIX_RGBA8 = 1, PFV_PIX_BGRA8 = 2 };
PFV_API size_t pfv_rgb_row_bytes(int width, int format);                       /* 0 for a bad format (or width <= 0) */
/* asynchronous on the context's stream */
PFV_API int pfv_frames_to_rgb_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src_dev, int src_layout, size_t src_stride,
                                  uint8_t *dst_dev, int format, size_t dst_pitch, size_t dst_stride);
/* host buffers: PACKED in, tight pictures out; synchronises; PFV_ERR_STATE while a graph is being recorded */
PFV_API int pfv_frames_to_rgb(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src, uint8_t *dst, int format);
/* A decoder session's pictures: always the conversion of what pfv_dec_get_frame_dev would return at that moment -- with pfv_dec_set_deblock
 * on, of the filtered picture (k_deblock into the planar output when a decode call has one, else into scratch of the session, then
 * k_present_rgb from that packed frame; a fused kernel is not offered).  The scratch is allocated by whichever of pfv_dec_set_deblock /
 * pfv_dec_set_output_rgb_dev / pfv_dec_get_frame_rgb* first needs it, never by a decode call (PFV_ERR_STATE if that moment lies inside a graph
 * recording).
 *   pfv_dec_get_frame_rgb_dev   all slots, pictures `stride` apart, asynchronous
 *   pfv_dec_get_frame_rgb       all slots, tight, to host memory; synchronises; PFV_ERR_STATE while a graph is being recorded
 *   pfv_dec_set_output_rgb_dev  an output IN ADDITION to the planar ones (pfv_dec_set_output_dev / _strided_dev and pfv_dec_get_frame* work
 *                               unchanged beside it): while set, every pfv_dec_iframe* / pfv_dec_pframe* call (dense, sparse, lists) also
 *                               writes the pictures of the slots of its window, indexed by slot, in one k_present_rgb from the new current
 *                               framebuffer.  dst_dev NULL switches it off; the framebuffer and the planar outputs are bit for bit what they
 *                               are without it.
 * pfv_gop_decoder and pfv_batch_decoder have no switch of their own: pass their device frames to pfv_frames_to_rgb_dev. */
PFV_API int pfv_dec_get_frame_rgb_dev(pfv_dec_session *s, uint8_t *dst_dev, int format, size_t pitch, size_t stride);
PFV_API int pfv_dec_get_frame_rgb(pfv_dec_session *s, uint8_t *dst_host, int format);
PFV_API int pfv_dec_set_output_rgb_dev(pfv_dec_session *s, uint8_t *dst_dev, int format, size_t pitch, size_t stride);
/* pfv_decoder: while on, the callback's y points to ONE tight picture in `format` and u, v are NULL -- in host memory, or in device memory
 * under pfv_decoder_set_output_device(1); lifetime as the planar frame's.  Results, order and errors of the advance calls are unchanged (a
 * drop-frame packet calls back as little as it does without the switch). */
PFV_API int pfv_decoder_set_output_rgb(pfv_decoder *d, int on, int format);

/* ------------------------------------------------------------------ RGB / RGBA picture input  [B]
 * The first step of an encoder, the mirror of the texture output: interleaved pixels as a renderer, a capture API or an image decoder hands
 * them over become the planar Y | U | V 4:2:0 frame every encoder entry point takes.  One launch, k_ingest_rgb
 * (csrc/pfv_ingest_kernels.hip), converts n_streams pictures.  Formats and byte orders: PFV_PIX_* above; the alpha byte of the 4-byte formats
 * is read and ignored, any value is accepted.
 * Source: rows `pitch` bytes apart (0 = pfv_rgb_row_bytes), pictures `stride` bytes apart (0 = pitch x height).
 * Destination: PACKED frames (Y | U | V as pfv_frame_bytes lays them out) `dst_stride` bytes apart (0 = pfv_frame_bytes).  Exactly the
 * frames' bytes are written: nothing between or beyond them.
 * Arithmetic (normative): the reference's load_frame (src/lib.rs:340-346).  For a pixel's bytes R, G, B as f32, in IEEE single precision,
 * evaluated left to right, every product and sum rounded on its own (no fused multiply-add):
 *     Y = ((0.299 * R) + (0.587 * G)) + (0.114 * B)
 *     U = ((128 - (0.168736 * R)) - (0.331264 * G)) + (0.5 * B)
 *     V = ((128 + (0.5 * R)) - (0.418688 * G)) - (0.081312 * B)
 * each converted as Rust's `as u8`: truncated toward zero, saturated to 0 .. 255.  These are the expressions of pfv_rgb_to_yuv420_dev.
 * The luma sample (x, y) is the pixel's Y.  The chroma sample (cx, cy) depends on the chroma mode:
 *   PFV_CHROMA_POINT  the U, V of pixel (2cx, 2cy): VideoFrame::from_planes -> reduce() (src/frame.rs:51-59), bit-identical to
 *                     pfv_rgb_to_yuv420_dev.  Three quarters of the chroma information are dropped, which aliases on fine colour detail.
 *   PFV_CHROMA_BOX    with a, b, c, d the u8 U (or V) values above of the four pixels (2cx + {0, 1}, 2cy + {0, 1}): (a + b + c + d + 2) >> 2
 *                     in integers.  Not in the reference.
 * Width and height are positive, even and fit u16.
 * A width that is a multiple of 8 with aligned operands -- source base, pitch and stride to 8 bytes for RGB8, to 16 for the 4-byte formats;
 * destination base and stride to 8 bytes -- takes 8- / 16-byte non-temporal loads, 8-byte luma and 4-byte chroma stores; anything else a
 * byte-granular path with the same result.  No atomics, nothing allocated: a call is one kernel node of a recorded graph.  Measured on one
 * MI355X: see profiles/ingest.md.
 * PFV_ERR_BAD_ARG: a format or chroma mode that does not exist, a null buffer or context, dimensions a frame cannot have, n_streams <= 0, a
 * pitch below the row size, a source stride below pitch x height, a destination stride below pfv_frame_bytes, source and destination ranges
 * that overlap. */
enum { PFV_CHROMA_POINT = 0, PFV_CHROMA_BOX = 1 };
/* asynchronous on the context's stream; one k_ingest_rgb */
PFV_API int pfv_frames_from_rgb_dev(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src_dev, int format, size_t src_pitch,
                                    size_t src_stride, uint8_t *dst_dev, size_t dst_stride, int chroma);
/* host buffers: tight pictures in, packed frames out; synchronises; PFV_ERR_STATE while a graph is being recorded */
PFV_API int pfv_frames_from_rgb(pfv_ctx *ctx, int width, int height, int n_streams, const uint8_t *src, uint8_t *dst, int format, int chroma);
/* An encoder session's input: the pictures of the slots of the session's current window (slot k's picture at pictures_dev + k * stride) into
 * slot k's frame of a packed buffer the session owns (n_streams x pfv_frame_bytes), one k_ingest_rgb; *frames_dev_out = that buffer's base.
 * From that point of the stream on the pointer is a valid `frames_dev` for every session entry point that takes one -- pfv_enc_iframe_dev /
 * pfv_enc_pframe_dev, the size / RD / SSIM probes, pfv_enc_distortion_dev, pfv_enc_ssim_dev -- indexed by slot as they index it, so one
 * ingest call serves all of them.  Frames of slots outside the window are left alone.  The buffer is allocated by the first call (which
 * returns PFV_ERR_STATE inside a graph recording; later calls are recorded as one kernel node) and lives with the session.
 * PFV_ERR_STATE while a non-zero pfv_enc_session_set_frame_stride is set: the buffer is packed.  GOP-batched input uses the picture
 * `stride` instead (G x picture bytes). */
PFV_API int pfv_enc_ingest_rgb_dev(pfv_enc_session *s, const uint8_t *pictures_dev, int format, size_t pitch, size_t stride, int chroma,
                                   const uint8_t **frames_dev_out);
/* pfv_encoder: while on, every call that takes (y, u, v) -- encode_iframe, encode_pframe, encode_frame and the six pfv_encoder_probe_* --
 * takes ONE tight host picture in `format` as y and requires u == v == NULL (anything else: PFV_ERR_BAD_ARG).  The picture goes up once into
 * device scratch of the encoder (made by this call, never by an encode call) and one k_ingest_rgb puts the frame into the session's frame
 * staging; the stream, the rungs chosen, frame types, reports and frame SSIM are bit for bit those of an encoder fed the converted planes.
 * `on` with a bad format or chroma mode: PFV_ERR_BAD_ARG; off ignores the other arguments and the calls are the planar ones again.
 * pfv_gop_encoder and pfv_batch_encoder have no switch of their own: their _dev forms take frames that pfv_frames_from_rgb_dev made. */
PFV_API int pfv_encoder_set_input_rgb(pfv_encoder *e, int on, int format, int chroma);

/* ------------------------------------------------------------------ frame resize  [B]
 * A frame sw x sh becomes a frame dw x dh without leaving the device: renditions of one source, thumbnails, a render-target size.  (The only
 * other resampling here, pfv_reduce_dev / pfv_double_dev, is the reference's point-sampled 2x pair, src/common.rs:523-556: one plane, one
 * ratio, aliasing by construction.)  One launch, k_scale (csrc/pfv_scale_kernels.hip), resizes n_streams frames, all three planes.
 * Arithmetic (normative).
 * Planes: all four sizes are positive, even and fit u16.  Each plane is resampled on its own by the same rule -- Y from sw x sh to dw x dh,
 * U and V from sw/2 x sh/2 to dw/2 x dh/2; chroma is treated as a centre-aligned plane like luma.  The filter is separable: per axis it maps
 * n_src samples to n_dst samples with a table.
 *   kind                  S   kernel K(t), a = |t|
 *   PFV_SCALE_BILINEAR    1   max(0, 1 - a)
 *   PFV_SCALE_BICUBIC     2   Catmull-Rom: a < 1: (1.5a - 2.5)*a*a + 1;  a < 2: ((-0.5a + 2.5)*a - 4)*a + 2;  else 0
 *   PFV_SCALE_LANCZOS3    3   K(0) = 1;  a < 3: sinc(pi*a) * sinc(pi*a / 3) with sinc(x) = sin(x) / x;  else 0
 * Table of one axis, built on the host in IEEE double, every operation rounded on its own (no fused multiply-add), expressions as written:
 *   m = max(n_src, n_dst);  f = n_src > n_dst ? n_src / n_dst : 1.0;  taps T = n_src > n_dst ? 2 * ceil(S * n_src / n_dst) : 2 * S (the
 *   ceiling in integers).  For the output index o, in exact integers: num = (2o + 1) * n_src - n_dst and
 *   first[o] = floor((num - 2 * S * m) / (2 * n_dst)) + 1, floor toward minus infinity.  Centre c = num / (2.0 * n_dst); weights
 *   w_k = K(((first[o] + k) - c) / f) for k = 0 .. T-1; their sum taken in that order, starting from w_0; q_k = rint(w_k / sum * 16384), ties
 *   to even; then 16384 - sum(q) is added to the tap of largest |q_k|, the first one on a tie.  Every row sums to exactly 16384.  Coefficients
 *   are int16, first is int32 and may be negative or reach past the end.  A row whose sum of |q_k| reaches 65536, or a coefficient outside
 *   int16, makes table creation return PFV_ERR_BAD_ARG; no size pair within the ratio limit is known to get there (the largest sum met over
 *   source sizes 2 .. 199 is 25 440, and 32767 * 25440 < 2^31: the sums below cannot leave i32).
 * Ratio limit: T <= 48, that is n_src <= 8 * n_dst on every axis of every plane; a larger reduction returns PFV_ERR_BAD_ARG and the caller
 * chains two calls.  Upscaling is limited only by u16.
 * Pixels: all values are i32, >> is an arithmetic shift (floor); indices are clamped to the PICTURE, 0 .. n_src-1, never to the padding of a
 * padded source:
 *   t[y][X]   = clamp((sum_k cx[X][k] * src[y][clampx(firstx[X] + k)] + 64) >> 7, -32768, 32767)        horizontal, every source row y
 *   out[Y][X] = clamp((sum_k cy[Y][k] * t[clampy(firsty[Y] + k)][X] + (1 << 20)) >> 21, 0, 255)          vertical
 * dw x dh == sw x sh reproduces the source byte for byte under all three kinds; a constant plane stays constant at every ratio.
 * Source: PACKED or PADDED frames with their own stream stride (the layout argument of pfv_frames_sse_dev), so a decoder session's
 * framebuffer is read where it lies.  Destination: PACKED frames dst_stride bytes apart (0 = pfv_frame_bytes(dw, dh)); exactly the
 * destination frames' bytes are written.  Both passes run in the one launch: a workgroup owns a 64 x 16 output tile, filters the source rows
 * it needs horizontally into LDS as 16-bit values and runs the vertical pass out of LDS -- no intermediate plane in HBM, no atomics, nothing
 * allocated by a run: a run is one kernel node of a recorded graph.  Planes whose rows all start on 4-byte boundaries (base, stream stride,
 * plane offset, row pitch) are read / written as dwords (non-temporal stores); anything else takes a byte-granular path with the same result.
 * PFV_ERR_BAD_ARG: a null pointer, n_streams <= 0, a kind or layout that does not exist, dimensions that are odd, non-positive or beyond
 * u16, a ratio beyond 8, strides below the frame size, source and destination ranges that overlap.
 * pfv_gop_* and pfv_batch_* objects have no switch: their _dev forms take frames that pfv_scaler_run_dev made. */
enum { PFV_SCALE_BILINEAR = 0, PFV_SCALE_BICUBIC = 1, PFV_SCALE_LANCZOS3 = 2 };
typedef struct pfv_scaler pfv_scaler;
PFV_API int pfv_scale_taps(int kind, int n_src, int n_dst);                  /* T, or 0 for bad arguments / a ratio beyond 8 */
/* host, no context: n_dst firsts, n_dst x T coefficients */
PFV_API int pfv_scale_table(int kind, int n_src, int n_dst, int32_t *first, int16_t *coef);
/* builds and uploads the four tables (luma x, luma y, chroma x, chroma y); NULL and *err on failure (err may be NULL); PFV_ERR_STATE inside a
 * graph recording.  The scaler belongs to the context and must be destroyed before it. */
PFV_API pfv_scaler *pfv_scaler_create(pfv_ctx *ctx, int sw, int sh, int dw, int dh, int kind, int *err);
PFV_API void pfv_scaler_destroy(pfv_scaler *sc);
/* asynchronous on the context's stream; one k_scale */
PFV_API int pfv_scaler_run_dev(pfv_scaler *sc, int n_streams, const uint8_t *src_dev, int src_layout, size_t src_stride, uint8_t *dst_dev,
                               size_t dst_stride);
/* host buffers: packed frames in, packed frames out; makes its tables, synchronises; PFV_ERR_STATE while a graph is being recorded */
PFV_API int pfv_frames_scale(pfv_ctx *ctx, int sw, int sh, int dw, int dh, int n_streams, const uint8_t *src, uint8_t *dst, int kind);
/* A decoder session's resized frames: an output IN ADDITION to the planar and RGB ones, exactly as pfv_dec_set_output_rgb_dev is.  While set,
 * every pfv_dec_iframe* / pfv_dec_pframe* call (dense, sparse, lists) also writes the resized frames of the slots of its window, indexed by
 * slot (slot k's frame at dst_dev + k * stride; stride 0 = pfv_frame_bytes of the destination size), in one k_scale from the new current
 * framebuffer -- with pfv_dec_set_deblock on from the filtered picture, taken from the planar output or from the session's scratch under the
 * RGB output's rule (one k_deblock serves both outputs; the scratch is made by the set calls, never by a decode call).  dst_dev NULL switches
 * it off.  The framebuffer and all other outputs stay bit for bit unchanged.  The scaler's source size must be the session's and its context
 * the session's, else PFV_ERR_BAD_ARG; the session does not own the scaler, which must outlive the setting. */
PFV_API int pfv_dec_set_output_scaled_dev(pfv_dec_session *s, pfv_scaler *sc, uint8_t *dst_dev, size_t stride);
/* pfv_decoder: w != 0: the callback's y, u, v point to the planes of ONE packed w x h frame (u == y + w*h, v == u + (w/2)*(h/2)), the decoded
 * -- and, if switched on, deblocked -- frame resized with `kind`, and its width / height arguments are w and h; on the host, or on the device
 * under pfv_decoder_set_output_device(1).  With pfv_decoder_set_output_rgb also on, the picture is the conversion of that resized frame:
 * k_scale, then k_present_rgb from the packed result.  pfv_decoder_width / _height keep reporting the stream's size.  w == 0 switches it off
 * (h and kind are then ignored).  Scratch is created by the set calls, never by an advance call.  Results, order and errors of the advance calls
 * are unchanged. */
PFV_API int pfv_decoder_set_output_size(pfv_decoder *d, int w, int h, int kind);
/* An encoder session's input, the mirror of pfv_enc_ingest_rgb_dev: the source frames (packed, of the scaler's source size) of the slots of the
 * session's current window -- slot k's at frames_dev + k * src_stride, 0 = pfv_frame_bytes of the source size -- are resized into slot k's
 * frame of a packed buffer the session owns (n_streams x pfv_frame_bytes), one k_scale; *frames_dev_out = that buffer's base, from that point
 * of the stream on a valid `frames_dev` for every session entry point that takes one.  Frames of slots outside the window are left alone.  The
 * buffer is a second one beside pfv_enc_ingest_rgb_dev's, allocated by the first call (PFV_ERR_STATE inside a graph recording; later calls
 * are recorded as one kernel node).  PFV_ERR_STATE while a non-zero pfv_enc_session_set_frame_stride is set.  The scaler's destination size
 * must be the session's and its context the session's, else PFV_ERR_BAD_ARG. */
PFV_API int pfv_enc_scale_dev(pfv_enc_session *s, pfv_scaler *sc, const uint8_t *frames_dev, size_t src_stride, const uint8_t **frames_dev_out);
/* pfv_encoder: src_w != 0: every call that takes (y, u, v) -- encode_iframe, encode_pframe, encode_frame and the six pfv_encoder_probe_* --
 * takes planes of the size src_w x src_h; they go up once into device scratch of the encoder (made by this call) and one k_scale puts the frame
 * into the session's frame staging.  With pfv_encoder_set_input_rgb also on, the picture is of the source size: it is ingested into that
 * scratch and scaled from there.  The stream, the rungs chosen, frame types, reports and frame SSIM are bit for bit those of an encoder fed
 * the frames that pfv_frames_scale made.  src_w == 0 switches it off (src_h and kind are then ignored). */
PFV_API int pfv_encoder_set_input_size(pfv_encoder *e, int src_w, int src_h, int kind);

/* ------------------------------------------------------------------ denoising pre-filter  [B]
 * k_enc_pframe skips a macroblock only when its best match lies below min_err, and an inter residual is quantised coarsely: sensor or grain
 * noise of a few grey levels turns static areas from skipped macroblocks into coded ones, at every rung.  The format has no loop filter and no
 * per-macroblock quantiser, so a PRE-filter on the encoder's input is the only lever -- and it keeps every parity with the reference: the
 * stream is byte for byte that of the reference encoder fed the filtered frames.  The mirror of the out-of-loop deblocking above.  Off by
 * default.
 *
 * The filter (normative).  Each plane of w x h 8-bit samples is filtered on its own, in i32 integers.  Two strengths per plane (Y, U, V), each
 * 0 .. 16: spatial Ss and temporal St.  The ramp is the deblocking filter's shape -- full up to S, back to zero at 2S, so real edges and motion
 * are left alone:
 *     phi(d, S) = sign(d) * max(0, |d| - max(0, 2 * (|d| - S)))        phi(d, 0) = 0
 *   Stage 1, spatial.   For the sample c at (x, y) and its eight neighbours n_k of the INPUT plane, with weights g = 2 for the four edge
 *                       neighbours and g = 1 for the four diagonal ones; a neighbour outside w x h contributes 0 (the padding of a padded
 *                       source never takes part):
 *                           s = c + ((sum_k g_k * phi(n_k - c, Ss) + 8) >> 4)            >> arithmetic (floor)
 *                       s lies between the minimum and the maximum of the 3 x 3 window: no clamp.  Stage 1 reads only the input, so it is
 *                       order-free and independent of the launch shape.
 *   Stage 2, temporal.  P is the stream's state at (x, y), the previous OUTPUT of this filter; tdiv truncates toward zero:
 *                           out = s + tdiv(3 * phi(P - s, St), 4)                          lies between s and P: no clamp
 *                       A stream that is not primed (after create or reset) skips stage 2: out = s.  A committed run writes `out` to the
 *                       destination AND to the state and primes the stream; an uncommitted run writes only the destination and leaves
 *                       state and priming alone.  Stage 2 is pointwise: the state is updated in place.
 * Ss == St == 0: out equals the input byte for byte.  A constant plane stays constant; identical consecutive frames with St > 0 converge to
 * themselves.
 * One launch, k_denoise (csrc/pfv_denoise_kernels.hip), covers all planes of n streams.  Source: PACKED or PADDED frames with their own
 * stream stride (pfv_frames_sse_dev); destination: PACKED frames dst_stride bytes apart (0 = back to back); exactly the frames' bytes are
 * written.  16-byte stores where aligned, a byte path with the same result otherwise.  No atomics, a run allocates nothing.  The streams'
 * `primed` flags live in device memory: create and reset clear them with stream-ordered memsets, a committed run that covers an unprimed
 * stream sets its window's flags with a stream-ordered memset behind the kernel.  A steady-state run is therefore exactly one kernel node of a
 * recorded graph; a run that would need that memset inside a graph recording returns PFV_ERR_STATE.  Measured on one MI355X: see
 * profiles/denoise.md. */
typedef struct pfv_denoiser pfv_denoiser;
/* owns the state (n_streams x pfv_frame_bytes) and the flags; strengths start at 0.  NULL and *err on failure (err may be NULL); PFV_ERR_STATE
 * inside a graph recording.  The denoiser belongs to the context and must be destroyed before it. */
PFV_API pfv_denoiser *pfv_denoiser_create(pfv_ctx *ctx, int width, int height, int n_streams, int *err);
PFV_API void pfv_denoiser_destroy(pfv_denoiser *dn);
/* per plane (Y, U, V), for the runs that follow; a value above 16: PFV_ERR_BAD_ARG */
PFV_API int pfv_denoiser_set_strength(pfv_denoiser *dn, const uint8_t spatial[3], const uint8_t temporal[3]);
/* un-primes streams [first_stream, first_stream + n); stream-ordered */
PFV_API int pfv_denoiser_reset(pfv_denoiser *dn, int first_stream, int n);
/* streams [first_stream, first_stream + n): stream first_stream + k's frame is at src_dev + k * src_stride and dst_dev + k * dst_stride (0 =
 * back to back in the layout).  Asynchronous on the context's stream.  PFV_ERR_BAD_ARG: a null pointer, a window outside n_streams, a layout
 * that does not exist, strides below the frame size, source and destination ranges that overlap, either overlapping the state. */
PFV_API int pfv_denoiser_run_dev(pfv_denoiser *dn, int first_stream, int n, const uint8_t *src_dev, int src_layout, size_t src_stride, uint8_t *dst_dev,
                                 size_t dst_stride, int commit);
/* host buffers, packed, frame-major ([frame][stream]): makes a denoiser, runs the frames in order, committed, and synchronises;
 * PFV_ERR_STATE while a graph is being recorded */
PFV_API int pfv_frames_denoise(pfv_ctx *ctx, int width, int height, int n_streams, int n_frames, const uint8_t *src, uint8_t *dst, const uint8_t spatial[3],
                               const uint8_t temporal[3]);
/* An encoder session's input, the mirror of pfv_enc_scale_dev: the frames (packed) of the slots of the session's current window -- slot k's at
 * frames_dev + k * src_stride, 0 = pfv_frame_bytes -- are filtered as the denoiser's streams k into slot k's frame of a third packed buffer the
 * session owns (n_streams x pfv_frame_bytes), one k_denoise; *frames_dev_out = that buffer's base, from that point of the stream on a valid
 * `frames_dev` for every session entry point that takes one.  Frames of slots outside the window are left alone.  The buffer is allocated by
 * the first call (PFV_ERR_STATE inside a graph recording).  PFV_ERR_STATE while a non-zero pfv_enc_session_set_frame_stride is set.  The
 * denoiser's size, stream count and context must be the session's, else PFV_ERR_BAD_ARG; the session does not own the denoiser.
 * pfv_gop_encoder and pfv_batch_encoder have no switch: their _dev forms take frames that pfv_denoiser_run_dev made. */
PFV_API int pfv_enc_denoise_dev(pfv_enc_session *s, pfv_denoiser *dn, const uint8_t *frames_dev, size_t src_stride, int commit, const uint8_t **frames_dev_out);
/* pfv_encoder: the last input stage, behind pfv_encoder_set_input_rgb and pfv_encoder_set_input_size: upload -> ingest -> scale -> denoise ->
 * the session's frame staging.  Scratch and the denoiser (one stream, owned) are made by this call, never by an encode call.  The frame an
 * encode_iframe / encode_pframe / encode_frame call uploads is filtered COMMITTED -- once per call: the budget and floor probes those calls run
 * work on the staged, filtered frame -- and the frame one of the six pfv_encoder_probe_* calls uploads is filtered UNCOMMITTED, so a probe
 * followed by the encode of the same picture shows the encoder the frame the probe saw.  The host entropy path brings the filtered planes back
 * down as it does for RGB / resized input.  The stream, the rungs chosen, frame types, reports and frame SSIM are bit for bit those of an
 * encoder fed the frames that pfv_frames_denoise makes of the same sequence.  Switching on (from off) un-primes the filter; `on` while on only
 * changes the strengths.  A strength above 16 or null strengths with `on`: PFV_ERR_BAD_ARG.  Off ignores the strengths, and every call is what
 * it is without the switch. */
PFV_API int pfv_encoder_set_denoise(pfv_encoder *e, int on, const uint8_t spatial[3], const uint8_t temporal[3]);

/* ------------------------------------------------------------------ exhaustive motion search  [B]
 * The reference chooses a macroblock's vector with a four-step logarithmic search (src/common.rs:154-204: steps 8, 4, 2, 1, 33 candidates), which
 * walks down one slope of the error surface and stops in a local minimum on textured content or large motion.  PFV_SEARCH_FULL looks at every
 * vector instead.  It is a MODE of an encoder session, not a PFV_OPT_*: its streams are ordinary .pfv streams that every decoder takes, but they
 * are not the reference encoder's bytes.  Default PFV_SEARCH_FOURSTEP: no launch and no byte differs from a session without this call.
 *
 * The rule (normative), for the macroblock at origin (bx, by) of a plane padded to pw x ph, against the session's previous reconstruction, with
 * radius R in 1 .. 15:
 *   candidates   all (dx, dy) with |dx| <= R, |dy| <= R, 0 <= bx + dx <= pw - 16, 0 <= by + dy <= ph - 16 (the bounds of src/common.rs:171, :182);
 *   E(dx, dy)    the exact integer sum of squared differences over the 16 x 16 block, at most 256 * 255^2 < 2^24: equal to the f32 value the
 *                reference compares;
 *   chosen       the lexicographic minimum of (E, |dx| + |dy|, dy, dx): (0, 0) wins every tie it takes part in, among equal errors the
 *                shortest vector wins, then the smallest dy, then the smallest dx.
 * Everything behind the choice is the existing operator: has_coef = !((float)E <= px_err^2 * 256) at the launch's rung; a skipped macroblock
 * has zero coefficients and the patch as its reconstruction; a coded one is clip(src - patch, +-255) -> encode_subblock_delta -> closed-loop
 * decode_block_delta.
 * Two launches: k_pf_search_full (csrc/pfv_fullsearch_kernels.hip) and k_pf_transform on the coded macroblocks.  One lane mapping at every grid
 * size: PFV_OPT_LANE_MAPPING and PFV_OPT_TILE_COMPACTION do not apply, PFV_OPT_ENC_TRANSFORM still selects the transform's form.  The outputs have
 * the four-step launch's layout, so rungs, windows, frame strides, by-reference slots, the ingest / scale / denoise stages, the device entropy
 * stage and the distortion / SSIM reports work unchanged.  Cost: profiles/full_search.md.
 * The mode applies to the p-frame launches that follow, like pfv_enc_session_set_rung; a launch recorded in a graph keeps the mode at capture
 * time.  radius: 1 .. 15 for FULL, ignored for FOURSTEP (reads back as 0).  An unknown mode or a radius outside 1 .. 15: PFV_ERR_BAD_ARG, and the
 * mode stays as it was.
 * The p-frame probes restate the four-step front end: while a session is in FULL mode pfv_enc_probe_pframe{,_rd,_ssim}{,_dev} return
 * PFV_ERR_STATE (so do pfv_encoder_probe_pframe*).  pfv_encoder_set_motion_search(FULL) is refused with PFV_ERR_STATE while
 * pfv_encoder_set_pframe_probe, pfv_encoder_set_pframe_quality_floor or pfv_encoder_set_pframe_ssim_floor is on, switching one of those on is
 * refused while FULL is on, and pfv_encoder_encode_frame returns PFV_ERR_STATE in FULL mode.  pfv_encoder_set_rate, the rungs and the i-frame
 * probes, budget and floors are unaffected.  pfv_gop_encoder: a batch that is made again (arena outgrown) takes the encoder's mode;
 * a change while a batch is in flight is refused with PFV_ERR_STATE (pfv_gop_encoder_flush first).  pfv_batch_encoder and the plane operator
 * pfv_encode_plane_delta have no switch. */
enum { PFV_SEARCH_FOURSTEP = 0, PFV_SEARCH_FULL = 1, PFV_SEARCH_HIER = 2 };
PFV_API int pfv_enc_session_set_motion_search(pfv_enc_session *s, int mode, int radius);
PFV_API int pfv_enc_session_get_motion_search(pfv_enc_session *s, int *mode, int *radius);   /* either pointer may be NULL */
PFV_API int pfv_encoder_set_motion_search(pfv_encoder *e, int mode, int radius);
/* pfv_gop_encoder_set_motion_search: with the GOP encoder below */

/* ------------------------------------------------------------------ wide-range hierarchical motion search  [B]
 * The format writes a vector component as a 7-bit two's-complement field (src/enc.rs:421-446, src/dec.rs:367-368): -64 .. 63 pixels.  The
 * four-step search and PFV_SEARCH_FULL stop at +-15.  PFV_SEARCH_HIER = 2 is a third MODE of the three setters above: a coarse search on
 * planes of half the size, then a fine search round twice the coarse vector.  Like FULL its streams are ordinary .pfv streams but not the
 * reference encoder's bytes, and with the mode off no launch and no byte changes.
 * radius: EVEN, 2 .. 62 -- the coarse level's reach in full-resolution pixels, Rc = radius / 2.  Anything else: PFV_ERR_BAD_ARG, the mode
 * stays as it was.  _get_motion_search reads back (2, radius).
 *
 * The rule (normative), per plane (Y, U, V are searched independently), the plane padded to pw x ph.  S is the padded source: the plane
 * inside w x h, the plane's clear value outside.  P is the session's previous reconstruction.
 *   1. half planes   hS[y][x] = (S[2y][2x] + S[2y][2x+1] + S[2y+1][2x] + S[2y+1][2x+1] + 2) >> 2, of size pw/2 x ph/2; hP from P likewise.
 *   2. coarse level  for the macroblock at (bx, by): the 8 x 8 block of hS at (bx/2, by/2); candidates all (cx, cy) with |cx|, |cy| <= Rc,
 *                    0 <= bx/2 + cx <= pw/2 - 8, 0 <= by/2 + cy <= ph/2 - 8; Ec the exact integer SSD over the 64 pixels (< 2^22); chosen
 *                    c = the lexicographic minimum of (Ec, |cx| + |cy|, cy, cx).
 *   3. fine level    at full resolution: candidates (0, 0) and every (2cx + rx, 2cy + ry) with |rx|, |ry| <= 2; each must satisfy
 *                    |dx|, |dy| <= 63 and lie inside the plane (0 <= bx + dx <= pw - 16, 0 <= by + dy <= ph - 16); E the exact 16 x 16 SSD as
 *                    in FULL; chosen = the lexicographic minimum of (E, |dx| + |dy|, dy, dx).  So E <= E(0, 0) always.
 *   4. behind the choice the existing operator, exactly as in FULL: has_coef = !((float)E <= px_err^2 * 256) at the launch's rung; a
 *      skipped macroblock has zero coefficients and the patch as its reconstruction; a coded one goes to k_pf_transform.
 * Launches (csrc/pfv_hiersearch_kernels.hip): k_halve on the source and on the reference, k_pf_search_coarse, k_pf_refine, k_pf_transform.
 * The outputs have the four-step launch's layout: rungs, windows, frame strides, by-reference slots, the ingest / scale / denoise stages,
 * the device entropy stage and the distortion / SSIM reports work unchanged.  Cost: profiles/hier_search.md.
 * The half planes and the coarse vectors are session scratch, allocated by the set_motion_search(HIER) call for all slots (PFV_ERR_NOMEM:
 * the mode stays as it was), never inside an encode call, and freed by pfv_enc_session_destroy.
 * Everything FULL refuses HIER refuses the same way (PFV_ERR_STATE): the p-frame probes, pfv_encoder_set_pframe_probe and the p-frame
 * quality / SSIM floors in both directions, pfv_encoder_encode_frame, a change on a pfv_gop_encoder with a batch in flight.
 * [C] pfv_enc_session_coarse_vectors: the coarse vectors (step 2) of the last p-frame launch over the current window, int8
 * [slot][macroblock][2], n_bytes = 2 * macroblocks * slots of the window; waits for the stream.  PFV_ERR_STATE when the last p-frame launch
 * was not a HIER one. */
PFV_API int pfv_enc_session_coarse_vectors(pfv_enc_session *s, int8_t *out, size_t n_bytes);
/* [C] pfv_enc_pframe_dev of a session in HIER mode (PFV_ERR_STATE otherwise) with an event in front of every kernel and behind the last; waits.
 * ms_out[5]: k_halve of the source, k_halve of the reference, k_pf_search_coarse, k_pf_refine, k_pf_transform.  tools/rd_curve.py --time-search. */
PFV_API int pfv_enc_pframe_hier_timed_dev(pfv_enc_session *s, const uint8_t *frames_dev, int8_t *mv_dev, uint8_t *has_coef_dev, int16_t *coef_dev, float ms_out[5]);

/* ------------------------------------------------------------------ quality ladder, p-frame byte budget  [B]
 * The format lets a header carry any number of q-tables and every packet name its three tables by index (src/dec.rs:89-111, :244-246); the
 * reference's encoder writes four tables and one quality for the whole stream.  A LADDER is several qualities in one stream: `qualities`
 * holds n_rungs values in 0..10, strictly ascending (1 <= n_rungs <= 11; a higher quality number is a coarser quantiser, src/enc.rs:40-51, so
 * rung 0 is the finest), rung r owns tables 4r .. 4r + 3 (intra_l, intra_c, inter_l, inter_c) and the px_err of qualities[r].  The rung is a
 * property of a launch: it applies to every slot of the encode / pack calls that follow pfv_enc_session_set_rung.  A ladder of one rung is
 * pfv_enc_session_create / pfv_encoder_create, byte for byte.  pfv_batch_encoder and pfv_gop_encoder keep one quality. */
PFV_API int pfv_enc_session_create_ladder(pfv_ctx *ctx, int width, int height, const int *qualities, int n_rungs, int n_streams,
                                          pfv_enc_session **out);
/* A launch recorded in a graph (pfv_graph_begin) keeps the table pointer, min_err and packet indices of the rung at capture time:
 * pfv_enc_session_set_rung does not reach the replays of an existing graph. */
PFV_API int pfv_enc_session_set_rung(pfv_enc_session *s, int rung);       /* PFV_ERR_BAD_ARG outside [0, n_rungs) */
PFV_API int pfv_enc_session_rung(pfv_enc_session *s);                     /* the current rung */
PFV_API int pfv_enc_session_rungs(pfv_enc_session *s);                    /* n_rungs */
/* pfv_encoder with a ladder: the header carries 4 * n_rungs tables, rung-major; pfv_encoder_create is the one-rung case. */
PFV_API int pfv_encoder_create_ladder(pfv_ctx *ctx, int width, int height, int framerate, const int *qualities, int n_rungs, pfv_encoder **out);
PFV_API int pfv_encoder_set_rung(pfv_encoder *e, int rung);               /* the rung of the frames that follow, on both entropy paths */
PFV_API int pfv_encoder_rung(pfv_encoder *e);                             /* of the last frame written; before the first frame the current rung */
PFV_API int pfv_encoder_rungs(pfv_encoder *e);
/* A p-frame byte budget in payload bytes (the packet adds 5), 0 = off.  One state variable, the current rung (rung 0 is the finest).
 * A p-frame is encoded at the current rung; with n = its payload bytes: n > pframe_budget moves the rung one step coarser, otherwise
 * 2 n <= pframe_budget one step finer, clamped to the ladder -- soft by one frame.  The factor 2 is a design constant (hysteresis wider
 * than the step between neighbouring qualities), not a measurement.  I-frames, drop frames and failed calls leave the rung alone;
 * pfv_encoder_set_rung may still be called and simply sets the state.  An i-frame's rung is chosen by size with pfv_encoder_set_iframe_budget
 * (below): the rung it picks is where this rule goes on from. */
PFV_API int pfv_encoder_set_rate(pfv_encoder *e, uint32_t pframe_budget);

/* ------------------------------------------------------------------ i-frame size probe, i-frame byte budget  [B]
 * payload bytes (the packet adds 5) that pfv_enc_iframe_dev + the entropy stage would produce for these frames at EVERY rung of the
 * session, from one read of the frames.  Reads no session state but the tables, window and frame stride; changes none: prev_frame, the
 * ping-pong index and the current rung stay as they are.  sizes_dev: uint32[n_streams][n_rungs], entries of slots outside the window left
 * alone; 0xffffffff = not encodable at that rung.  stats_dev (may be NULL): uint32[n_streams][n_rungs][17], the 16 symbol counts and the
 * sum of coefficient sizes (undefined where the size is 0xffffffff).  Asynchronous on the context's stream; recordable in a graph (scratch
 * rule as pfv_frames_sse_dev: the session's accumulator is allocated by the first call, so call once before pfv_graph_begin).  Two launches,
 * k_probe_iframe + k_probe_sizes (csrc/pfv_probe_kernels.hip); no host-side clear, no host synchronisation. */
PFV_API int pfv_enc_probe_iframe_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev);
PFV_API int pfv_enc_probe_iframe(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out);      /* host buffers, all slots, packed; synchronises */
PFV_API int pfv_encoder_probe_iframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out /*[n_rungs]*/);
/* I-frame byte budget in payload bytes, 0 = off (default: today's behaviour, byte for byte).  On: encode_iframe probes the frame first and
 * encodes it at the FINEST rung whose payload fits the budget, or the coarsest rung if none does (a scan from rung 0 -- sizes need not be
 * monotone); that rung becomes the current rung, so the p-frames behind it and pfv_encoder_set_rate's rule start from it.  Costs one extra
 * launch pair and one 4 * n_rungs-byte download (with its synchronisation) per i-frame, on both entropy paths; the frame goes up once.  A
 * one-rung encoder has nothing to choose and does not probe. */
PFV_API int pfv_encoder_set_iframe_budget(pfv_encoder *e, uint32_t iframe_budget);

/* ------------------------------------------------------------------ i-frame rate-distortion probe, i-frame quality floor  [B]
 * A finer rung does not always look better: decode indexes SCALE and q by zigzag position, encode by raster position (src/dct.rs:78-82
 * against :92-93), so PSNR is not monotone over the ladder and a rung can cost more bytes AND more error than its coarser neighbour.  This
 * probe measures: from ONE read of the frames, per slot of the window and EVERY rung, the payload size and counts exactly as
 * pfv_enc_probe_iframe_dev defines them and the squared error per plane exactly as pfv_frames_sse_dev defines it between the frame and the
 * reconstruction pfv_enc_iframe_dev at that rung would leave in prev_frame (only pixels inside the plane's w x h count).
 *   sizes_dev  uint32[n_streams][n_rungs]; sse_dev  uint64[n_streams][n_rungs][3] (Y, U, V; undefined where the size is 0xffffffff);
 *   stats_dev  uint32[n_streams][n_rungs][17] or NULL.
 * Contract of pfv_enc_probe_iframe_dev: reads the tables, the window and the frame stride, changes nothing, leaves the entries of slots
 * outside the window alone, asynchronous on the context's stream, recordable (the first call allocates the accumulators: call once before
 * pfv_graph_begin, inside a recording it returns PFV_ERR_STATE).  Two launches, k_probe_iframe_rd + k_probe_rd_sizes
 * (csrc/pfv_rdprobe_kernels.hip); no host-side clear, no host synchronisation. */
PFV_API int pfv_enc_probe_iframe_rd_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev);
PFV_API int pfv_enc_probe_iframe_rd(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out);   /* host buffers, all slots, packed; synchronises */
PFV_API int pfv_encoder_probe_iframe_rd(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out /*[n_rungs]*/,
                                        uint64_t *sse_out /*[n_rungs][3]*/);
/* I-frame quality floor in dB of PSNR-YUV as pfv_frame_report.psnr_yuv defines it, 0 = off (default: today's behaviour, byte for byte, the
 * i-frame budget's rule included).  On, with more than one rung: encode_iframe (and pfv_encoder_encode_frame through it) runs the
 * rate-distortion probe in place of the size probe.  ALLOWED are the rungs that are encodable and, if an i-frame budget is set, within it;
 * none allowed: the coarsest rung.  Of the allowed rungs with psnr_yuv >= min_psnr_yuv the one with the FEWEST bytes is taken, ties to the
 * lower index; if none reaches the floor, the allowed rung with the smallest total squared error, ties to fewer bytes, then to the lower
 * index.  That rung becomes the current rung.  +INFINITY is legal ("the best-looking rung that fits"); NaN and negative values return
 * PFV_ERR_BAD_ARG.  Costs one launch pair, one download of 28 * n_rungs bytes and one synchronisation per i-frame; the frame goes up once. */
PFV_API int pfv_encoder_set_iframe_quality_floor(pfv_encoder *e, double min_psnr_yuv);

/* ------------------------------------------------------------------ p-frame size probe, hard p-frame budget, automatic frame type  [B]
 * payload bytes (the packet adds 5) that pfv_enc_pframe_dev + the entropy stage would produce for these frames against the session's CURRENT
 * prev_frame at EVERY rung, from one motion search and one forward transform of the residual: the search does not depend on the rung, only
 * the skip test and the quantiser do.  Reads the tables, the window, the frame stride and prev_frame; changes nothing: prev_frame, the
 * ping-pong index and the current rung stay as they are.  sizes_dev: uint32[n_streams][n_rungs], entries of slots outside the window left
 * alone; 0xffffffff = not encodable at that rung.  stats_dev (may be NULL): uint32[n_streams][n_rungs][PFV_PPROBE_STATS] (undefined where
 * the size is 0xffffffff).  A frame without a coded macroblock has an all-zero histogram and (152 + header bits + 7) / 8 bytes.
 * Asynchronous on the context's stream; recordable in a graph (the scratch rule of pfv_enc_probe_iframe_dev: the first call allocates, so it
 * returns PFV_ERR_STATE inside a recording).  Two launches, k_probe_pframe (csrc/pfv_pprobe_kernels.hip) + k_pprobe_sizes; no host-side
 * clear, no host synchronisation.  One lane mapping, 8 lanes per macroblock: PFV_OPT_LANE_MAPPING does not apply. */
enum { PFV_PPROBE_STATS = 20 };   /* 16 symbol counts, sum coeff_size, coded mbs, mbs with mv != 0, header bits */
PFV_API int pfv_enc_probe_pframe_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint32_t *stats_dev);
PFV_API int pfv_enc_probe_pframe(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out);      /* host buffers, all slots, packed; synchronises */
/* pfv_encoder: the same against the encoder's reference; no state changes.  PFV_ERR_STATE when the encoder is poisoned or finished, as
 * pfv_encoder_encode_pframe. */
PFV_API int pfv_encoder_probe_pframe(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out /*[n_rungs]*/);
/* Hard p-frame budget, default 0 = off (today's behaviour, byte for byte).  With on != 0, a pfv_encoder_set_rate budget != 0 and more than
 * one rung, encode_pframe probes the frame first and encodes it at the FINEST rung whose payload is <= the budget (a scan from rung 0; a rung
 * marked 0xffffffff does not fit), or at the coarsest rung if none fits; that rung becomes the current rung and the soft rule of
 * pfv_encoder_set_rate is not applied while the probe is on.  Costs one launch pair, one 4 * n_rungs-byte download and one synchronisation
 * per p-frame, on both entropy paths; the frame goes up once. */
PFV_API int pfv_encoder_set_pframe_probe(pfv_encoder *e, int on);
/* pfv_encoder_encode_frame chooses the frame's type; *type_out (may be NULL): 1 i-frame, 2 p-frame, 3 drop frame.  In this order:
 *   1. a forced i-frame (encode_iframe's path, i-frame budget included) when no frame has been written yet, or the encoder is poisoned, or
 *      max_interval > 0 (pfv_encoder_set_gop; default 0 = never; < 0: PFV_ERR_BAD_ARG) and max_interval frames, drop frames included, have
 *      followed the last i-frame;
 *   2. the frame goes up once and is sized as a p-frame; rp = the hard budget's rung where that applies, else the current rung;
 *   3. no coded macroblock at rp and no non-zero vector: a drop frame (it shows the frame that p-frame would show and leaves the same
 *      reference); the rung stays;
 *   4. the frame is sized as an i-frame from the same upload; isize[rp] <= psize[rp]: an i-frame, its rung chosen as encode_iframe does;
 *   5. otherwise a p-frame at rp, which becomes the current rung.
 * Costs per frame behind the first: up to two launch pairs, two downloads of at most 84 * n_rungs and 4 * n_rungs bytes, each with its
 * synchronisation, before the encode itself.  Rule 4 means what it says and is NOT a scene-cut detector: residuals are halved
 * (src/common.rs:118-119, :304), so a p-frame across a cut is often the smaller one (texture, noise) and is then written.  Frame reports
 * work as for the explicit calls.  pfv_gop_encoder and pfv_batch_encoder keep one quality and have none of this.  The detector is a switch
 * of its own, pfv_encoder_set_scene_cut ("scene-cut detection", below): it adds rule 1b and serves the other two objects as a look-ahead.
 *   4 with the p-frame quality floor on (pfv_encoder_set_pframe_quality_floor, below; rules 1 to 3 stay, rp = the floor's rung): the frame is
 *      measured as an i-frame by the rate-distortion probe from the same upload; ri = the rung encode_iframe would choose with its own budget and
 *      floor settings, from these results (no second probe, no second upload).  The candidates are the p-frame at rp and the i-frame at ri; each
 *      MEETS when its PSNR-YUV is at or above the P-FRAME floor.  Exactly one meets: that one.  Both meet: the one with fewer bytes, ties to the
 *      i-frame (today's <=).  Neither meets: the smaller total squared error, ties to fewer bytes, then to the i-frame.  A candidate that is
 *      not encodable never meets and loses to one that is.  The i-frame is written at ri, the p-frame at rp; either becomes the current rung. */
PFV_API int pfv_encoder_set_gop(pfv_encoder *e, int max_interval);
PFV_API int pfv_encoder_encode_frame(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, int *type_out /* 1 i, 2 p, 3 drop */);

/* ------------------------------------------------------------------ scene-cut detection  [B]
 * A cheap look-ahead measure between "frames in HBM" and "which of them start a GOP": how well the previous frame predicts this one, against how
 * much this one varies in itself.  A zero-motion difference is not enough (a pan scores like a cut), so the measure holds a small motion
 * search at quarter resolution.  Integer, order-free, many frames or streams per launch.  Fades, flashes and chroma are out of scope.
 *
 * The measure (normative).  Luma only; `prev` and `cur` are two frames of w x h; everything is exact integer arithmetic.
 *   Quarter planes.  qw = w >> 2, qh = h >> 2.  Q[y][x] = (sum of the 4 x 4 luma pixels at (4x, 4y) + 8) >> 4.  Pixels beyond 4 qw / 4 qh and
 *                    any padding never take part.
 *   Blocks.          nbx = qw >> 3, nby = qh >> 3 blocks of 8 x 8 quarter samples (32 x 32 pixels).  Quarter samples beyond 8 nbx / 8 nby belong
 *                    to no block as the CURRENT block, but a candidate may cover them.  n_blocks = nbx * nby may be 0.
 *   Intra.           Per block B of Qcur at (8bx, 8by): mean = (sum B + 32) >> 6, intra = sum |B - mean|  (<= 16 320).
 *   Inter.           The candidates are all (cx, cy) with |cx|, |cy| <= R, 0 <= 8bx + cx <= qw - 8 and 0 <= 8by + cy <= qh - 8.  S(cx, cy) is the
 *                    SAD of B against the 8 x 8 block of Qprev at (8bx + cx, 8by + cy).  The chosen candidate is the lexicographic minimum of
 *                    (S, |cx| + |cy|, cy, cx) -- the project's tie rule.  best = S(chosen), zero = S(0, 0).  The radius R is 0 .. 7 quarter
 *                    samples (+-4R pixels); the default 4 matches the four-step search's +-15; R = 0 is zero motion only.
 *   Per pair of frames, pfv_scene_stats (40 bytes): inter = sum best, intra = sum intra, zero = sum zero over the blocks; n_blocks (0 when the
 *                    stream has no previous frame: every other field is then 0 too); n_intra = blocks with best >= intra; n_moving = blocks
 *                    whose chosen vector is not (0, 0); reserved = 0.  Every entry is written by every run: no atomics, nothing to clear.
 *   Per block maps (diagnostics, [C]): uint32 best << 16 | intra, and int8[2] = the chosen (cx, cy).
 * Three kernels (csrc/pfv_scene_kernels.hip): k_scene_quarter (frames -> u8 quarter planes; PACKED or PADDED operand with its own stream stride,
 * 16-byte loads where legal and a byte path with the same result otherwise), k_scene_cost (one wavefront per block, the window of Qprev in LDS,
 * one lane per candidate, v_sad_u8, the tie rule as the minimum of one packed key) and k_scene_sum (the map summed per pair, 64-bit).  Measured
 * on one MI355X: profiles/scene_cut.md. */
typedef struct pfv_scene_stats {
    uint64_t inter, intra, zero;
    uint32_t n_blocks, n_intra, n_moving, reserved;
} pfv_scene_stats;
enum { PFV_SCENE_RADIUS_DEFAULT = 4, PFV_SCENE_THRESHOLD_DEFAULT = 176 };
/* Pure host functions.  The score in q8: 0 when n_blocks == 0, else min(65535, inter * 256 / max(intra, 64 * n_blocks)), floor division; the
 * 64 * n_blocks floor keeps flat or black frames from dividing by nothing (black -> black is 0, black <-> picture is large).  The default
 * threshold 176 is the geometric mean of the largest continuous score and the smallest cut score of synthetic clips at R = 5
 * (profiles/scene_cut.md); nobody has measured real footage, and the threshold is the caller's argument. */
PFV_API uint32_t pfv_scene_score_q8(const pfv_scene_stats *stats);
/* types_out[k] = 1 (i-frame) or 2 (p-frame) for stats[0 .. n_frames), returns the number of i-frames.  Frame 0 is an i-frame.  With d = k - (the
 * index of the last i-frame): frame k is an i-frame when max_interval > 0 && d >= max_interval, or when score(stats[k]) >= threshold_q8 &&
 * d >= max(1, min_interval); every other frame is a p-frame.  Null pointers, n_frames <= 0 or a negative interval: PFV_ERR_BAD_ARG. */
PFV_API int pfv_scene_plan(const pfv_scene_stats *stats, int n_frames, uint32_t threshold_q8, int min_interval, int max_interval, uint8_t *types_out);
/* The detector owns, per stream, the previous quarter plane (the state) and a `primed` flag in device memory (handled as pfv_denoiser handles
 * its own: create and reset clear them with stream-ordered memsets, a committed run over an unprimed stream sets its window's flags with a
 * memset behind the kernels), quarter scratch for max(n_streams, max_clip_frames) frames and the block maps.  Width and height positive, even,
 * <= 65535; n_streams >= 1; max_clip_frames >= 0.  NULL and *err on failure (err may be NULL); PFV_ERR_STATE inside a graph recording.  Destroy
 * it before its context. */
typedef struct pfv_scene_detector pfv_scene_detector;
PFV_API pfv_scene_detector *pfv_scene_detector_create(pfv_ctx *ctx, int width, int height, int n_streams, int max_clip_frames, int *err);
PFV_API void pfv_scene_detector_destroy(pfv_scene_detector *det);
/* R for the runs that follow; outside 0 .. 7: PFV_ERR_BAD_ARG and the radius stays as it was */
PFV_API int pfv_scene_detector_set_radius(pfv_scene_detector *det, int radius);
/* un-primes streams [first_stream, first_stream + n); stream-ordered */
PFV_API int pfv_scene_detector_reset(pfv_scene_detector *det, int first_stream, int n);
/* Frame t of streams [first_stream, first_stream + n) in one launch group (three kernels), asynchronous on the context's stream: stream
 * first_stream + k's frame is at src_dev + k * src_stride (0 = back to back in the layout) and is measured against that stream's state into
 * stats_dev[k] (device memory, 8-byte aligned).  Streams outside the window are left alone.  With commit the current quarter planes become the
 * state through a stream-ordered copy and the streams are primed; an uncommitted run leaves state and priming alone.  A steady-state run is
 * recordable; a run that must set `primed` flags inside a graph recording returns PFV_ERR_STATE.  PFV_ERR_BAD_ARG: a null pointer, a window
 * outside n_streams, a layout that does not exist, a stride below the layout's frame size, a misaligned stats_dev -- nothing is written. */
PFV_API int pfv_scene_detector_run_dev(pfv_scene_detector *det, int first_stream, int n, const uint8_t *src_dev, int src_layout, size_t src_stride, int commit,
                                       pfv_scene_stats *stats_dev /*[n]*/);
/* n_frames <= max_clip_frames consecutive frames of ONE stream, frame k at frames_dev + k * stride, in one launch group: entry 0 is measured
 * against the stream's state, entry k against frame k - 1; with commit the last frame becomes the state.  The results are bit for bit those of
 * n_frames committed run_dev calls on that stream.  The recipe for pfv_gop_encoder, which needs its GOP boundaries before anything is encoded:
 * measure the clip in HBM once, pfv_scene_plan, then feed pfv_gop_encoder_encode_iframe_dev / _pframe_dev by the plan. */
PFV_API int pfv_scene_detector_run_clip_dev(pfv_scene_detector *det, int stream, int n_frames, const uint8_t *frames_dev, int layout, size_t stride, int commit,
                                            pfv_scene_stats *stats_dev /*[n_frames]*/);
/* [C] the block maps of the last run, entries [first, first + n) -- run_dev: stream indices, run_clip_dev: frame indices -- each
 * n_blocks = ((w >> 2) >> 3) * ((h >> 2) >> 3) long; either pointer may be NULL; waits for the stream */
PFV_API int pfv_scene_detector_maps(pfv_scene_detector *det, int first, int n, uint32_t *blk_out, int8_t *vec_out);
/* [C] measurement only: an UNCOMMITTED run_dev (clip == 0: streams [first, first + n)) or run_clip_dev (clip != 0: n frames of stream `first`)
 * with an event between the kernels; synchronises.  ms_out: k_scene_quarter, k_scene_cost, k_scene_sum.  PFV_ERR_STATE inside a graph recording. */
PFV_API int pfv_scene_detector_run_timed_dev(pfv_scene_detector *det, int first, int n, int clip, const uint8_t *src_dev, int layout, size_t stride,
                                             pfv_scene_stats *stats_dev, float ms_out[3]);
/* host frames, packed, frame-major ([frame][stream]): makes a detector, runs the frames in order, committed, and synchronises; stats_out
 * [n_frames][n_streams]; the mirror of pfv_frames_denoise.  PFV_ERR_STATE while a graph is being recorded */
PFV_API int pfv_frames_scene(pfv_ctx *ctx, int width, int height, int n_streams, int n_frames, const uint8_t *frames, int radius, pfv_scene_stats *stats_out);
/* pfv_encoder: cut-aware frame types.  The detector (one stream, owned) and its scratch are made by this call, never by an encode call; radius
 * 0 .. 7 and min_interval >= 0, else PFV_ERR_BAD_ARG; switching on (from off) un-primes the detector.
 * ON: every encode_iframe / encode_pframe / encode_frame call measures the STAGED frame (behind ingest -> scale -> denoise) committed, once per
 * call; the six pfv_encoder_probe_* calls measure uncommitted; encode_dropframe leaves the state alone.  The frame goes up once per call.
 * pfv_encoder_encode_frame gains rule 1b between rules 1 and 2: score >= threshold_q8 and at least max(1, min_interval) frames, drop frames
 * included, have followed the last i-frame, this frame counted (d of pfv_scene_plan: an i-frame directly behind an i-frame is possible unless
 * min_interval >= 2): an i-frame, its rung chosen as encode_iframe chooses it; no p-frame sizing runs.  Otherwise rules 2 - 5 apply as they are.  With PFV_SEARCH_FULL / PFV_SEARCH_HIER and the switch on, encode_frame no longer
 * returns PFV_ERR_STATE: rule 1, rule 1b, else a p-frame at the current rung -- no sizing, no drop frames.  Costs one launch group, one 40-byte
 * download and one synchronisation per frame.
 * OFF (the default, or after on = 0): no launch, no byte and no return code differs from an encoder without the switch, PFV_ERR_STATE from
 * encode_frame in FULL / HIER mode included. */
PFV_API int pfv_encoder_set_scene_cut(pfv_encoder *e, int on, uint32_t threshold_q8, int radius, int min_interval);
/* the stats of the last call that measured; PFV_ERR_STATE when the switch is off or no frame has been measured */
PFV_API int pfv_encoder_last_scene(pfv_encoder *e, pfv_scene_stats *out);

/* ------------------------------------------------------------------ p-frame rate-distortion probe, p-frame quality floor  [B]
 * A p-frame is often the smaller frame AND the worse-looking one: residuals are halved, and a skipped macroblock costs no bytes whatever its
 * error.  This probe measures: from ONE motion search and ONE forward transform of the residual, per slot of the window and EVERY rung, the
 * payload size and counts exactly as pfv_enc_probe_pframe_dev defines them and the squared error per plane exactly as pfv_frames_sse_dev
 * defines it between the frame and the reconstruction pfv_enc_pframe_dev at that rung would leave in prev_frame (only pixels inside the
 * plane's w x h count; a skipped macroblock reconstructs to its patch).
 *   sizes_dev  uint32[n_streams][n_rungs]; sse_dev  uint64[n_streams][n_rungs][3] (Y, U, V; undefined where the size is 0xffffffff);
 *   stats_dev  uint32[n_streams][n_rungs][PFV_PPROBE_STATS] or NULL.
 * Contract of pfv_enc_probe_pframe_dev: reads the tables, the window, the frame stride and prev_frame, changes nothing (prev_frame, the
 * ping-pong index and the current rung stay as they are), leaves the entries of slots outside the window alone, asynchronous on the context's
 * stream, recordable (the first call allocates the accumulators: call once before pfv_graph_begin, inside a recording it returns
 * PFV_ERR_STATE).  Two launches, k_probe_pframe_rd + k_pprobe_rd_sizes (csrc/pfv_prdprobe_kernels.hip); no host-side clear, no host
 * synchronisation.  One lane mapping, 8 lanes per macroblock. */
PFV_API int pfv_enc_probe_pframe_rd_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev, uint32_t *stats_dev);
PFV_API int pfv_enc_probe_pframe_rd(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out);   /* host buffers, all slots, packed; synchronises */
/* pfv_encoder: the same against the encoder's reference; no state changes.  PFV_ERR_STATE when the encoder is poisoned or finished. */
PFV_API int pfv_encoder_probe_pframe_rd(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out /*[n_rungs]*/,
                                        uint64_t *sse_out /*[n_rungs][3]*/);
/* P-frame quality floor in dB of PSNR-YUV as pfv_frame_report.psnr_yuv defines it, 0 = off (default: today's behaviour, byte for byte).  On,
 * with more than one rung: encode_pframe runs the rate-distortion probe and chooses by the i-frame floor's rule.  ALLOWED are the rungs that
 * are encodable and, if a pfv_encoder_set_rate budget is set, within it -- with the floor on that budget is a hard cap whether or not
 * pfv_encoder_set_pframe_probe is on, and the soft rule is not applied; none allowed: the coarsest rung.  Of the allowed rungs with
 * psnr_yuv >= min_psnr_yuv the one with the FEWEST bytes is taken, ties to the lower index; if none reaches the floor, the allowed rung with
 * the smallest total squared error, ties to fewer bytes, then to the lower index.  That rung becomes the current rung.  +INFINITY is legal;
 * NaN and negative values return PFV_ERR_BAD_ARG.  pfv_encoder_encode_frame: rule 4 above changes with the floor on.  Costs one launch pair,
 * one download of 28 * n_rungs bytes and one synchronisation per p-frame; the frame goes up once. */
PFV_API int pfv_encoder_set_pframe_quality_floor(pfv_encoder *e, double min_psnr_yuv);

/* ------------------------------------------------------------------ SSIM probe, i- and p-frame SSIM floors  [B]
 * Squared error rates the blocking of a coarse rung far too kindly, and the two metrics do rank the rungs of this codec differently.  The
 * SSIM probes are the rate-distortion probes with one more result: per slot of the window and EVERY rung
 *   sizes_dev, sse_dev, stats_dev   exactly what pfv_enc_probe_iframe_rd_dev / pfv_enc_probe_pframe_rd_dev define (stats_dev may be NULL);
 *   ssim_q24_dev   int64[n_streams][n_rungs][3] (Y, U, V): per plane the sum of q exactly as pfv_frames_ssim_dev defines it, between the frame
 *                  and the reconstruction that pfv_enc_iframe_dev / pfv_enc_pframe_dev at that rung would leave in prev_frame (a skipped
 *                  macroblock reconstructs to its patch).  The window count per plane is pfv_ssim_windows; a plane without windows reports 0.
 *                  Undefined where the size is 0xffffffff.  The values are the ones pfv_enc_ssim_dev returns behind a real encode at that
 *                  rung, bit for bit: the same integers through the same window function.
 * Everything else is the rate-distortion probes' contract: the call changes nothing (prev_frame, the ping-pong index, the current rung),
 * leaves the entries of slots outside the window alone, honours the frame stride, is asynchronous on the context's stream and recordable
 * after one unrecorded call (the first call allocates; inside a recording it returns PFV_ERR_STATE); the host-buffer forms work on all
 * slots, packed, and synchronise.
 * Three launches (csrc/pfv_ssimprobe_kernels.hip): k_probe_iframe_ssim or k_probe_pframe_ssim leaves the 4 x 4 block sums of every rung in
 * a map, k_probe_ssim_windows forms every window from its four blocks and writes the plane sums through a fixed reduction, and the RD
 * probes' own tail (k_probe_rd_sizes / k_pprobe_rd_sizes) stays a launch of its own.  No host-side clear, no host synchronisation.
 * Scratch: the map takes n_streams * pfv_total_blocks * (n_rungs * 128 + 64) bytes (1080p, 11 rungs: 18 MB per stream), allocated by the
 * first call, freed with the session. */
PFV_API int pfv_enc_probe_iframe_ssim_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev,
                                          int64_t *ssim_q24_dev, uint32_t *stats_dev /* may be NULL */);
PFV_API int pfv_enc_probe_iframe_ssim(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out, int64_t *ssim_q24_out);   /* host buffers, all slots, packed; synchronises */
PFV_API int pfv_enc_probe_pframe_ssim_dev(pfv_enc_session *s, const uint8_t *frames_dev, uint32_t *sizes_dev, uint64_t *sse_dev,
                                          int64_t *ssim_q24_dev, uint32_t *stats_dev /* may be NULL */);
PFV_API int pfv_enc_probe_pframe_ssim(pfv_enc_session *s, const uint8_t *frames, uint32_t *sizes_out, uint64_t *sse_out, int64_t *ssim_q24_out);   /* host buffers, all slots, packed; synchronises */
/* pfv_encoder: the same for one frame, as an i-frame or against the encoder's reference; no state changes.  The p-frame form returns
 * PFV_ERR_STATE when the encoder is poisoned or finished. */
PFV_API int pfv_encoder_probe_iframe_ssim(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out /*[n_rungs]*/,
                                          uint64_t *sse_out /*[n_rungs][3]*/, int64_t *ssim_q24_out /*[n_rungs][3]*/);
PFV_API int pfv_encoder_probe_pframe_ssim(pfv_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t *sizes_out /*[n_rungs]*/,
                                          uint64_t *sse_out /*[n_rungs][3]*/, int64_t *ssim_q24_out /*[n_rungs][3]*/);
/* SSIM floors: min_ssim is the mean SSIM of the frame as pfv_frame_ssim.ssim_all defines it.  0 = off (default: today's behaviour, byte for
 * byte); values in (0, 1] are legal, 1 meaning "the best-looking rung that fits"; NaN, negative values and values above 1 return
 * PFV_ERR_BAD_ARG.  With a floor of that frame type on and more than one rung, encode_iframe / encode_pframe run the SSIM probe in place of
 * the size or rate-distortion probe: one launch group, one download of 52 * n_rungs bytes, one synchronisation; the frame goes up once.
 *   ALLOWED as without it: the rung is encodable and within the i-frame budget / the pfv_encoder_set_rate budget (for p-frames a hard cap;
 *   the soft rule is not applied); none allowed: the coarsest rung.
 *   A rung MEETS when it is allowed, meets the PSNR floor of that frame type if one is on, and
 *   pfv_ssim(q24[Y] + q24[U] + q24[V], windows) >= min_ssim.  A frame without any window meets every SSIM floor.
 *   Of the rungs that meet, the one with the FEWEST bytes, ties to the lower index.  If none meets and the frame has windows: the allowed
 *   rung with the largest q24 total, ties to the smaller total squared error, then fewer bytes, then the lower index.  (Without windows the
 *   PSNR floor's rule decides.)  The chosen rung becomes the current rung.
 * pfv_encoder_encode_frame with either kind of p-frame floor on takes rule 4 in its floor form: rp is the floors' rung; the i-frame is
 * measured from the same upload, by the SSIM probe if the i-frame or the p-frame SSIM floor is on; ri is encode_iframe's own choice from
 * those results; a candidate MEETS by the p-frame floors that are on.  Exactly one meets: that one.  Both: fewer bytes, ties to the i-frame.
 * Neither, the p-frame SSIM floor on and windows: the larger q24 total, then the smaller squared error, then fewer bytes, then the i-frame;
 * otherwise neither-meets is the PSNR floor's rule.  pfv_gop_encoder and pfv_batch_encoder keep one quality and have no floors. */
PFV_API int pfv_encoder_set_iframe_ssim_floor(pfv_encoder *e, double min_ssim);
PFV_API int pfv_encoder_set_pframe_ssim_floor(pfv_encoder *e, double min_ssim);

/* ------------------------------------------------------------------ batch encoder (n streams per step, pipelined)  [B]
 * n independent streams of one geometry encoded together -- the reference runs one Encoder per stream (src/enc.rs:12-26);
 * every writer receives exactly the bytes an Encoder of its own would have written.  Per frame step: ONE upload of all
 * frames (on a copy stream, overlapping the host-side collection of the previous step), one kernel launch per stage for
 * all streams, one download of all payloads.  Packets reach the writers one step late; finish flushes.
 *   write != NULL: called with each stream's header / packets in stream order (from the thread calling encode / finish);
 *   write == NULL: the library keeps each stream's bytes until pfv_batch_encoder_take hands them over. */
typedef struct pfv_batch_encoder pfv_batch_encoder;
typedef void (*pfv_write_cb)(void *user, int stream, const uint8_t *data, size_t len);
PFV_API int pfv_batch_encoder_create(pfv_ctx *ctx, int width, int height, int framerate, int quality, int n_streams,
                                     pfv_write_cb write, void *user, pfv_batch_encoder **out);
/* page-locked [n_streams][pfv_frame_bytes] array to fill for the NEXT encode call (two alternate; valid for that call only) */
PFV_API uint8_t *pfv_batch_encoder_frames(pfv_batch_encoder *b);
/* one frame step for all streams.  frames == NULL: the array from pfv_batch_encoder_frames; else the caller's own
 * [n_streams][frame_bytes] buffer (ideally from pfv_host_alloc), free again when the call returns.  pframe: 0 = i-frames
 * (Encoder::encode_iframe, src/enc.rs:75-123), 1 = p-frames (:125-173).  Returns when the step is enqueued. */
PFV_API int pfv_batch_encoder_encode(pfv_batch_encoder *b, int pframe, const uint8_t *frames);
PFV_API int pfv_batch_encoder_flush(pfv_batch_encoder *b);
PFV_API int pfv_batch_encoder_finish(pfv_batch_encoder *b);
PFV_API int pfv_batch_encoder_take(pfv_batch_encoder *b, int stream, const uint8_t **data, size_t *len);
PFV_API void pfv_batch_encoder_destroy(pfv_batch_encoder *b);

/* ------------------------------------------------------------------ batch decoder (n streams per step, pipelined)  [B]
 * n `.pfv` byte streams of one geometry and one packet-type pattern decoded together: per step the packets are bit-parsed on
 * n_threads worker threads (one task per stream; 0 = on the calling thread), one kernel launch decodes all streams, one copy
 * brings the frames back; the parse of step t+1 overlaps the device work of step t.  `streams[k]` must stay valid while the
 * decoder lives (the reference's R: Read + Seek).  Frames, their order and the error codes are those of n independent
 * Decoder::advance_frame loops (src/dec.rs:169-224) run in lockstep. */
typedef struct pfv_batch_decoder pfv_batch_decoder;
PFV_API int pfv_batch_decoder_create(pfv_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n_streams, int n_threads,
                                     pfv_batch_decoder **out);
PFV_API int pfv_batch_decoder_width(const pfv_batch_decoder *b);
PFV_API int pfv_batch_decoder_height(const pfv_batch_decoder *b);
PFV_API int pfv_batch_decoder_framerate(const pfv_batch_decoder *b);
/* steps so far whose coefficient lists overflowed (more than 1 non-zero in 4) and were parsed / uploaded in the dense form */
PFV_API long pfv_batch_decoder_dense_steps(const pfv_batch_decoder *b);
/* as pfv_decoder_entropy_counts: a step whose payloads reach 64 KiB (every step under PFV_ENTROPY_DECODE_DEVICE) goes through the device's
 * entropy stage, the pool then only reads tables and block headers */
PFV_API void pfv_batch_decoder_entropy_counts(const pfv_batch_decoder *b, long counts_out[2]);
/* 1: *frames_out = [n_streams][pfv_frame_bytes] decoded frames (page-locked, valid until the call after next); 2: a step of drop
 * frames; 0: end of the streams; negative: error (PFV_ERR_FORMAT also when packet types or q-table indices diverge between streams) */
PFV_API int pfv_batch_decoder_advance(pfv_batch_decoder *b, const uint8_t **frames_out);
PFV_API void pfv_batch_decoder_destroy(pfv_batch_decoder *b);

/* ------------------------------------------------------------------ GOP-batched encoder / decoder of ONE stream  [B]
 * enc::Encoder (src/enc.rs:12-188) and dec::Decoder (src/dec.rs:15-224) with the same calls, bytes and frames as pfv_encoder /
 * pfv_decoder, but with the independent GOPs of the stream as the slots of every kernel launch: encode_iframe never reads
 * prev_frame and overwrites every plane of it (src/enc.rs:84-97), decode_plane_into overwrites the framebuffer
 * (src/common.rs:477-496), so the runs I P P ... of one stream can be worked on side by side -- frame t of every run of a batch
 * in ONE launch per stage.  A single 4K stream then fills the device the way 20 streams do.
 *   max_gops        runs ("groups") per batch = slots per launch; a group starts at every i-frame
 *   max_gop_frames  frames of a group inside one batch; a longer run continues in the next batch (its reference frame is
 *                   carried over on the device), and so does a stream that starts with p-frames
 *   payload_budget  device bytes for the packet payloads of one batch.  0: twice the batch's raw frame bytes (real content stays below
 *                   1.6 x); a batch that outgrows that all the same is encoded again frame by frame and the arena grows -- like
 *                   Encoder::encode_pframe (src/enc.rs:125-173) the object cannot fail for size.  An explicit budget is kept as given:
 *                   PFV_ERR_NOMEM from the call that completes a batch whose payloads do not fit it
 * Encoder: the planes may be reused when an encode call returns; frames are uploaded on a copy stream while the kernels of the
 * previous batch run.  A packet reaches pfv_gop_encoder_drain when its batch is complete (max_gops groups seen, flush, finish);
 * the byte stream is the one pfv_encoder writes.  After an error the stream is incomplete and every call returns PFV_ERR_STATE.
 * Decoder: one scan of the packet headers (type:u8, len:u32, src/dec.rs:179-180) cuts a batch.  The packet payloads are read
 * either on the DEVICE (PFV_OPT_ENTROPY_DECODE, the default when the batch's coefficient arrays fit: the host only reads each
 * packet's table, q indices and block headers -- n_threads workers + the caller -- and the run streams are read by the k_entd_*
 * kernels, step t + 1 on streams of their own while step t is decoded and its frames travel to the host) or by the host parser
 * pool (the packets of a frame step bit-parsed in parallel, step t + 1 under the device work of step t).  Frames are delivered in
 * stream order, with the results (1 / 0 / error) the sequential loop gives call by call -- a packet that does not parse leaves
 * the framebuffer alone, and the frames behind a failed i-frame decode against the previous run's last frame, as they do there.
 * y / u / v of the callback are one packed frame (u == y + w*h, v == u + (w/2)*(h/2)) and stay valid until the call that starts
 * the next batch.
 * GOP boundaries: the encoder runs one stream's GOPs side by side, so they must be known before anything is encoded; it has no switch for
 * that.  The recipe: measure the clip where it lies in HBM with pfv_scene_detector_run_clip_dev, turn the stats into frame types with
 * pfv_scene_plan (a fixed interval is its max_interval), and feed encode_iframe_dev / encode_pframe_dev by the plan. */
typedef struct pfv_gop_encoder pfv_gop_encoder;
typedef struct pfv_gop_decoder pfv_gop_decoder;
typedef struct pfv_iovec { const uint8_t *data; size_t len; } pfv_iovec;
PFV_API int pfv_gop_encoder_create(pfv_ctx *ctx, int width, int height, int framerate, int quality, int max_gops, int max_gop_frames,
                                   size_t payload_budget, pfv_gop_encoder **out);
PFV_API int pfv_gop_encoder_encode_iframe(pfv_gop_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v);
PFV_API int pfv_gop_encoder_encode_pframe(pfv_gop_encoder *e, const uint8_t *y, const uint8_t *u, const uint8_t *v);
/* the same for a packed frame (Y | U | V, pfv_frame_bytes) that already lies in DEVICE memory (frames a renderer or another kernel left in
 * HBM): nothing crosses PCIe on the way in.  Ordered on the context's stream like every *_dev call: the frame is read behind the work
 * enqueued there before the call and may be overwritten by work enqueued there after it; no host wait.  (The frame is COPIED on that stream
 * into the batch being filled; the batches' kernels run on a stream the encoder owns, so the copies of one batch run under the kernels of the
 * batch before it.  PFV_GOP_TRACE=1 in the environment: a host-side log of the encoder's submits, step downloads and arrivals on stderr.) */
PFV_API int pfv_gop_encoder_encode_iframe_dev(pfv_gop_encoder *e, const uint8_t *frame_dev);
PFV_API int pfv_gop_encoder_encode_pframe_dev(pfv_gop_encoder *e, const uint8_t *frame_dev);
/* on != 0: frames handed to the two calls above are taken BY REFERENCE -- the batch's kernels read them where they lie, no copy (16-byte
 * aligned frames; a misaligned one is copied as before).  The caller then promises that such a frame stays valid and unchanged until its batch
 * has been collected: until the packet of that frame has been handed out by pfv_gop_encoder_drain / _drain_iov, or pfv_gop_encoder_flush /
 * _finish has returned.  Same bytes.  (The frame-at-a-time contract of Encoder::encode_pframe, src/enc.rs:125 -- the frame is borrowed for
 * the call only -- is what forces the copy by default; a renderer that keeps a ring of frames does not need it.) */
PFV_API int pfv_gop_encoder_set_frames_by_reference(pfv_gop_encoder *e, int on);
/* the motion search of the batches submitted from now on ("exhaustive motion search" above); PFV_ERR_STATE while a batch is in flight */
PFV_API int pfv_gop_encoder_set_motion_search(pfv_gop_encoder *e, int mode, int radius);
PFV_API int pfv_gop_encoder_encode_dropframe(pfv_gop_encoder *e);
PFV_API int pfv_gop_encoder_flush(pfv_gop_encoder *e);
PFV_API int pfv_gop_encoder_finish(pfv_gop_encoder *e);
PFV_API int pfv_gop_encoder_drain(pfv_gop_encoder *e, const uint8_t **data, size_t *len);
PFV_API int pfv_gop_encoder_bytes(pfv_gop_encoder *e, const uint8_t **data, size_t *len);
/* the writer side without a copy: the bytes produced since the last drain as `count` segments in stream order (packet headers, and
 * payloads where the device-to-host copy put them, in page-locked memory) -- one write_all per segment, as the reference's W: Write
 * receives them (src/enc.rs:190-235).  Valid until the next call on this encoder. */
PFV_API int pfv_gop_encoder_drain_iov(pfv_gop_encoder *e, const pfv_iovec **iov, size_t *count);
PFV_API long pfv_gop_encoder_batches(const pfv_gop_encoder *e);
/* where the object's host time went, in seconds since creation (returns the number of entries written, <= n).
 * encoder: [0] waiting for plane uploads, [1] enqueueing batches, [2] waiting for a batch's kernels, [3] payloads device -> host,
 *          [4] packet assembly; counts: [5] device frames read by reference (pfv_gop_encoder_set_frames_by_reference), [6] batches that
 *          outgrew their payload arena and were encoded again
 * decoder: [0] header scan, [1] waiting for the packet parsers, [2] waiting for the device before a staging set is reused,
 *          [3] enqueueing, [4] waiting for a batch's last frames, [5] waiting for the device's entropy stage (PFV_OPT_ENTROPY_DECODE);
 *          counts: [6] packets whose payload the device read, [7] packets of such batches that were left to the host parser, of which
 *          [8] because the device's read had not settled within its rounds and [9] because it found the payload irregular;
 *          [10] host-parsed packets whose coefficient list outgrew its place in the pool and got a buffer of its own */
PFV_API int pfv_gop_encoder_stats(const pfv_gop_encoder *e, double *out, int n);
PFV_API void pfv_gop_encoder_destroy(pfv_gop_encoder *e);
PFV_API int pfv_gop_decoder_create(pfv_ctx *ctx, const uint8_t *data, size_t len, int max_gops, int max_gop_frames, int n_threads,
                                   pfv_gop_decoder **out);
PFV_API int pfv_gop_decoder_width(const pfv_gop_decoder *d);
PFV_API int pfv_gop_decoder_height(const pfv_gop_decoder *d);
PFV_API int pfv_gop_decoder_framerate(const pfv_gop_decoder *d);
PFV_API long pfv_gop_decoder_batches(const pfv_gop_decoder *d);
PFV_API int pfv_gop_decoder_stats(const pfv_gop_decoder *d, double *out, int n);
/* on != 0: decoded frames stay in device memory and the callback's y / u / v are DEVICE pointers (valid until the call that starts the
 * next batch; the context's stream is idle when the callback runs) -- for consumers on the GPU (the reference README's texture-out
 * wish, README.md:20): the download of the frames, the whole PCIe cost of decoding, is not paid.  Between batches only (PFV_ERR_STATE). */
PFV_API int pfv_gop_decoder_set_output_device(pfv_gop_decoder *d, int on);
/* Decoder::reset (src/dec.rs:148-152).  Like the reference's, it does not rewind the framebuffer; this decoder has decoded ahead of
 * the frames it delivered, so a stream whose first packet is a p-frame continues from the last DECODED frame after a reset. */
PFV_API int pfv_gop_decoder_reset(pfv_gop_decoder *d);
PFV_API int pfv_gop_decoder_advance_frame(pfv_gop_decoder *d, pfv_video_cb onvideo, void *user);
PFV_API int pfv_gop_decoder_advance_delta(pfv_gop_decoder *d, double delta, pfv_video_cb onvideo, void *user);
PFV_API void pfv_gop_decoder_destroy(pfv_gop_decoder *d);

/* packet payload serialisers alone (write_iframe_packet / write_pframe_packet bodies, src/enc.rs:237-320, 332-470);
 * return the payload size (0 on error); the payload is copied to `out` when it fits `cap` */
PFV_API size_t pfv_serialize_iframe_payload(const int16_t *coef, int total_blocks, uint8_t *out, size_t cap);
PFV_API size_t pfv_serialize_pframe_payload(const int8_t *mv, const uint8_t *has_coef, const int16_t *coef, int total_blocks,
                                            uint8_t *out, size_t cap);

/* packet payload parsers alone (the bit-reading halves of decode_iframe / decode_pframe, src/dec.rs:226-296, 328-417; host
 * only, no device): coef_out [total_blocks][256] is zero-filled first.  PFV_OK, PFV_ERR_FORMAT or PFV_ERR_IO. */
PFV_API int pfv_parse_iframe_payload(const uint8_t *payload, size_t len, int total_blocks, int n_qtables, int16_t *coef_out,
                                     uint8_t qidx_out[3]);
PFV_API int pfv_parse_pframe_payload(const uint8_t *payload, size_t len, int total_blocks, int n_qtables, int8_t *mv_out,
                                     uint8_t *has_coef_out, int16_t *coef_out, uint8_t qidx_out[3]);
/* same, into the (flat index, value) list pfv_dec_*_sparse take; returns 1 when more than `cap` pairs would be needed */
PFV_API int pfv_parse_payload_sparse(int is_pframe, const uint8_t *payload, size_t len, int total_blocks, int n_qtables,
                                     int8_t *mv_out, uint8_t *has_coef_out, uint32_t *idx_out, int16_t *val_out, size_t cap,
                                     size_t *n_out, uint8_t qidx_out[3]);
/* Packets are independent bit streams: up to n_threads of them are parsed (src/dec.rs:226-296, 328-417) ahead of the
 * one being decoded, on worker threads; 0 = parse inline.  Default min(4, hardware threads - 1).  Frames, their order
 * and the error returned by each advance call are those of the sequential loop (src/dec.rs:169-224). */
PFV_API int pfv_decoder_set_lookahead(pfv_decoder *d, int n_threads);
/* The run streams of a packet are read on the DEVICE (k_entd_*, see PFV_OPT_ENTROPY_DECODE: taken from the context when the decoder is
 * created) for payloads of 64 KiB and more -- every payload under PFV_ENTROPY_DECODE_DEVICE, none under _HOST; the look-ahead threads
 * then only read tables and block headers.  counts_out[0]: packets the device read so far, [1]: packets its stage was not certain
 * about and left to the host parser.  Same frames and results either way. */
PFV_API void pfv_decoder_entropy_counts(const pfv_decoder *d, long counts_out[2]);
/* on != 0: the decoded frame stays in device memory; the callback's y / u / v are DEVICE pointers to the packed frame (u == y + w*h,
 * v == u + (w/2)*(h/2)), valid until the next advance call (see pfv_gop_decoder_set_output_device) */
PFV_API int pfv_decoder_set_output_device(pfv_decoder *d, int on);

#ifdef __cplusplus
}
#endif
#endif /* PFV_HIP_EXT_H */
