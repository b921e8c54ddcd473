// pfv_hip.hpp -- C++ host classes over the C ABI of pfv_hip.h, with the reference's public surface:
//   pfv::VideoPlane  (src/plane.rs:1-36)     width, height, pixels  (public fields, tightly packed rows)
//   pfv::VideoFrame  (src/frame.rs:3-59)     width, height, plane_y / plane_u / plane_v
//   pfv::Encoder     (src/enc.rs:12-188)     new(writer, w, h, framerate, quality, num_threads) -> Encoder(writer, ..., Context&)
//   pfv::Decoder     (src/dec.rs:15-224)     new(reader, num_threads)                            -> Decoder(reader, Context&)
//   pfv::GopEncoder / pfv::GopDecoder        the same two objects with the independent GOPs of the stream as the slots of every launch
//                                            (pfv_gop_encoder / pfv_gop_decoder): same bytes, same frames, same results call by call
// The reference's `num_threads` slot (its rayon pool) is the pfv::Context: one device + one HIP stream.  Writers are
// std::ostream, readers std::istream (read to the end on construction; the reference needs Read + Seek).  Errors of the
// C ABI become pfv::Error (what() = pfv_last_error); DecodeError::{FormatError, VersionError, IOError} keep their codes.
// Header-only; link against libpfv_hip.so.
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <istream>
#include <iterator>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "pfv_hip.h"

namespace pfv {

class Error : public std::runtime_error {
  public:
    Error(int code, const std::string &what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }   // a pfv_status value

  private:
    int code_;
};

class Context {
  public:
    explicit Context(int device = 0)
    {
        int rc = pfv_ctx_create(device, &h_);
        if (rc != PFV_OK) throw Error(rc, last(nullptr));
    }
    ~Context() { pfv_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    pfv_ctx *handle() const { return h_; }
    void check(int rc) const
    {
        if (rc != PFV_OK) throw Error(rc, last(h_));
    }

  private:
    static std::string last(pfv_ctx *h)
    {
        const char *m = pfv_last_error(h);
        return m ? m : "pfv_hip error";
    }
    pfv_ctx *h_ = nullptr;
};

// src/plane.rs:1-36
struct VideoPlane {
    size_t width = 0, height = 0;
    std::vector<uint8_t> pixels;
    VideoPlane() = default;
    VideoPlane(size_t w, size_t h) : width(w), height(h), pixels(w * h, 0) {}                    // VideoPlane::new
    static VideoPlane from_slice(size_t w, size_t h, const uint8_t *data, size_t len)           // VideoPlane::from_slice
    {
        if (len != w * h) throw std::invalid_argument("VideoPlane::from_slice: len != width * height (src/plane.rs:14)");
        VideoPlane p;
        p.width = w; p.height = h;
        p.pixels.assign(data, data + len);
        return p;
    }
};

// src/frame.rs:3-26
struct VideoFrame {
    size_t width = 0, height = 0;
    VideoPlane plane_y, plane_u, plane_v;
    VideoFrame() = default;
    VideoFrame(size_t w, size_t h) : width(w), height(h), plane_y(w, h), plane_u(w / 2, h / 2), plane_v(w / 2, h / 2)   // VideoFrame::new
    {
        if (w % 2 || h % 2) throw std::invalid_argument("VideoFrame: width and height must be even (src/frame.rs:13)");
        plane_u.pixels.assign(plane_u.pixels.size(), 128);
        plane_v.pixels.assign(plane_v.pixels.size(), 128);
    }
};

// distortion (pfv_hip_ext.h, "distortion on the device"): 10 log10(255^2 n / sse); +inf for sse == 0, NaN for n == 0
inline double psnr(uint64_t sse, uint64_t n_samples) { return pfv_psnr(sse, n_samples); }
// what one Encoder::encode_* call wrote and how far its reconstruction is from the frame it was given (pfv_frame_report)
struct FrameReport {
    int type = 0;                    // 1 i-frame, 2 p-frame, 3 drop frame
    uint32_t packet_bytes = 0;       // 5-byte packet header + payload
    uint64_t sse[3] = {0, 0, 0};     // Y, U, V; zeros for a drop frame
    double psnr[3] = {0, 0, 0};
    double psnr_yuv = 0;
};

// structural similarity (pfv_hip_ext.h, "structural similarity on the device"): the mean of `windows` window values summed in 2^-24 fixed
// point; NaN for windows == 0
inline double ssim(int64_t q24_sum, uint64_t windows) { return pfv_ssim(q24_sum, windows); }
// SSIM windows per plane (Y, U, V) of a width x height frame
inline std::array<uint32_t, 3> ssim_windows(size_t width, size_t height)
{
    std::array<uint32_t, 3> out{};
    if (pfv_ssim_windows((int)width, (int)height, out.data()) != PFV_OK) throw Error(PFV_ERR_BAD_ARG, "ssim_windows: width/height must be positive, even and fit u16");
    return out;
}
// the structural similarity between the frame one Encoder::encode_* call was given and its reconstruction (pfv_frame_ssim)
struct FrameSsim {
    int64_t q24[3] = {0, 0, 0};      // Y, U, V; zeros for a drop frame
    uint32_t windows[3] = {0, 0, 0};
    double ssim[3] = {0, 0, 0};      // per plane
    double ssim_all = 0;             // over all windows of the frame
};

// out-of-loop deblocking (pfv_hip_ext.h, "out-of-loop deblocking"): the modes of Decoder::set_deblock, the automatic strength of a q-table
// (min(12, q[0] >> 1)), and the filter on packed Y|U|V frames in host memory at the strengths (Y, U, V), each 0..12
enum class Deblock { Off = PFV_DEBLOCK_OFF, Auto = PFV_DEBLOCK_AUTO, Fixed = PFV_DEBLOCK_FIXED };
inline int deblock_strength(const int32_t qtable[64]) { return pfv_deblock_strength(qtable); }
inline std::vector<uint8_t> frames_deblock(Context &ctx, size_t width, size_t height, const std::vector<uint8_t> &frames, const std::array<uint8_t, 3> &strength)
{
    const size_t fb = pfv_frame_bytes((int)width, (int)height);
    if (!fb || frames.empty() || frames.size() % fb) throw std::invalid_argument("frames_deblock: frames must hold whole packed frames");
    std::vector<uint8_t> out(frames.size());
    ctx.check(pfv_frames_deblock(ctx.handle(), (int)width, (int)height, (int)(frames.size() / fb), frames.data(), out.data(), strength.data()));
    return out;
}

// RGB / RGBA texture output (pfv_hip_ext.h, "RGB / RGBA texture output"): the pixel formats, and packed Y|U|V frames in host memory as tight
// interleaved pictures, back to back (the reference's save_frame arithmetic)
enum class PixelFormat { Rgb8 = PFV_PIX_RGB8, Rgba8 = PFV_PIX_RGBA8, Bgra8 = PFV_PIX_BGRA8 };
inline size_t rgb_row_bytes(size_t width, PixelFormat format) { return pfv_rgb_row_bytes((int)width, (int)format); }
inline std::vector<uint8_t> frames_to_rgb(Context &ctx, size_t width, size_t height, const std::vector<uint8_t> &frames, PixelFormat format)
{
    const size_t fb = pfv_frame_bytes((int)width, (int)height), row = rgb_row_bytes(width, format);
    if (!fb || frames.empty() || frames.size() % fb) throw std::invalid_argument("frames_to_rgb: frames must hold whole packed frames");
    std::vector<uint8_t> out(frames.size() / fb * row * height);
    ctx.check(pfv_frames_to_rgb(ctx.handle(), (int)width, (int)height, (int)(frames.size() / fb), frames.data(), out.data(), (int)format));
    return out;
}

// RGB / RGBA picture input (pfv_hip_ext.h, "RGB / RGBA picture input"): the chroma modes, and tight interleaved pictures in host memory, back
// to back, as packed Y|U|V frames (the reference's load_frame arithmetic; Box: the mean of the 2 x 2 pixels' chroma instead of the even pixel's)
enum class ChromaMode { Point = PFV_CHROMA_POINT, Box = PFV_CHROMA_BOX };
inline std::vector<uint8_t> frames_from_rgb(Context &ctx, size_t width, size_t height, const std::vector<uint8_t> &pictures, PixelFormat format,
                                            ChromaMode chroma = ChromaMode::Point)
{
    const size_t fb = pfv_frame_bytes((int)width, (int)height), pic = rgb_row_bytes(width, format) * height;
    if (!fb || !pic || pictures.empty() || pictures.size() % pic) throw std::invalid_argument("frames_from_rgb: pictures must hold whole tight pictures");
    std::vector<uint8_t> out(pictures.size() / pic * fb);
    ctx.check(pfv_frames_from_rgb(ctx.handle(), (int)width, (int)height, (int)(pictures.size() / pic), pictures.data(), out.data(), (int)format, (int)chroma));
    return out;
}

// src/enc.rs:12-188
// frame resize (include/pfv_hip_ext.h, "frame resize"): the filter kinds, one axis' table, the plan object and the host-buffer form
enum class ScaleKind { Bilinear = PFV_SCALE_BILINEAR, Bicubic = PFV_SCALE_BICUBIC, Lanczos3 = PFV_SCALE_LANCZOS3 };
inline int scale_taps(ScaleKind kind, size_t n_src, size_t n_dst) { return pfv_scale_taps((int)kind, (int)n_src, (int)n_dst); }
struct ScaleTable {
    int taps = 0;
    std::vector<int32_t> first;   // [n_dst]
    std::vector<int16_t> coef;    // [n_dst][taps]: every row sums to 16384
};
inline ScaleTable scale_table(ScaleKind kind, size_t n_src, size_t n_dst)
{
    ScaleTable t;
    t.taps = scale_taps(kind, n_src, n_dst);
    if (!t.taps) throw Error(PFV_ERR_BAD_ARG, "scale_table: a kind that does not exist, a size outside 1 .. 65535 or a reduction beyond 8");
    t.first.resize(n_dst);
    t.coef.resize(n_dst * (size_t)t.taps);
    const int rc = pfv_scale_table((int)kind, (int)n_src, (int)n_dst, t.first.data(), t.coef.data());
    if (rc != PFV_OK) throw Error(rc, pfv_last_error(nullptr));
    return t;
}
// pfv_scaler: the four tables of one (source size, destination size, kind) on the device; destroy it before its context
class Scaler {
  public:
    Scaler(Context &ctx, size_t sw, size_t sh, size_t dw, size_t dh, ScaleKind kind) : ctx_(ctx), sw_(sw), sh_(sh), dw_(dw), dh_(dh)
    {
        int rc = PFV_OK;
        h_ = pfv_scaler_create(ctx.handle(), (int)sw, (int)sh, (int)dw, (int)dh, (int)kind, &rc);
        if (!h_) ctx_.check(rc ? rc : PFV_ERR_BAD_ARG);
    }
    ~Scaler() { pfv_scaler_destroy(h_); }
    Scaler(const Scaler &) = delete;
    Scaler &operator=(const Scaler &) = delete;
    pfv_scaler *handle() const { return h_; }
    size_t src_frame_bytes() const { return pfv_frame_bytes((int)sw_, (int)sh_); }
    size_t dst_frame_bytes() const { return pfv_frame_bytes((int)dw_, (int)dh_); }
    // asynchronous on the context's stream, one k_scale: device frames in (packed or padded, src_stride apart), packed device frames out
    void run_dev(int n_streams, const uint8_t *src_dev, uint8_t *dst_dev, int src_layout = PFV_FRAME_PACKED, size_t src_stride = 0, size_t dst_stride = 0)
    {
        ctx_.check(pfv_scaler_run_dev(h_, n_streams, src_dev, src_layout, src_stride, dst_dev, dst_stride));
    }

  private:
    Context &ctx_;
    size_t sw_, sh_, dw_, dh_;
    pfv_scaler *h_ = nullptr;
};
inline std::vector<uint8_t> frames_scale(Context &ctx, size_t sw, size_t sh, size_t dw, size_t dh, const std::vector<uint8_t> &frames, ScaleKind kind)
{
    const size_t sfb = pfv_frame_bytes((int)sw, (int)sh), dfb = pfv_frame_bytes((int)dw, (int)dh);
    if (!sfb || !dfb || frames.empty() || frames.size() % sfb) throw std::invalid_argument("frames_scale: frames must hold whole packed frames of the source size");
    std::vector<uint8_t> out(frames.size() / sfb * dfb);
    ctx.check(pfv_frames_scale(ctx.handle(), (int)sw, (int)sh, (int)dw, (int)dh, (int)(frames.size() / sfb), frames.data(), out.data(), (int)kind));
    return out;
}

// pfv_denoiser (pfv_hip_ext.h, "denoising pre-filter"): the previous output and the primed flag of n_streams streams; destroy it before its context
class Denoiser {
  public:
    Denoiser(Context &ctx, size_t width, size_t height, int n_streams = 1) : ctx_(ctx), width_(width), height_(height), n_(n_streams)
    {
        int rc = PFV_OK;
        h_ = pfv_denoiser_create(ctx.handle(), (int)width, (int)height, n_streams, &rc);
        if (!h_) ctx_.check(rc ? rc : PFV_ERR_BAD_ARG);
    }
    ~Denoiser() { pfv_denoiser_destroy(h_); }
    Denoiser(const Denoiser &) = delete;
    Denoiser &operator=(const Denoiser &) = delete;
    pfv_denoiser *handle() const { return h_; }
    size_t frame_bytes() const { return pfv_frame_bytes((int)width_, (int)height_); }
    // per plane (Y, U, V), 0 .. 16, for the runs that follow
    void set_strength(const std::array<uint8_t, 3> &spatial, const std::array<uint8_t, 3> &temporal) { ctx_.check(pfv_denoiser_set_strength(h_, spatial.data(), temporal.data())); }
    void reset(int first_stream = 0, int n = -1) { ctx_.check(pfv_denoiser_reset(h_, first_stream, n < 0 ? n_ - first_stream : n)); }
    // asynchronous on the context's stream, one k_denoise: device frames in (packed or padded, src_stride apart), packed device frames out
    void run_dev(int first_stream, int n, const uint8_t *src_dev, uint8_t *dst_dev, bool commit = true, int src_layout = PFV_FRAME_PACKED, size_t src_stride = 0,
                 size_t dst_stride = 0)
    {
        ctx_.check(pfv_denoiser_run_dev(h_, first_stream, n, src_dev, src_layout, src_stride, dst_dev, dst_stride, commit ? 1 : 0));
    }

  private:
    Context &ctx_;
    size_t width_, height_;
    int n_;
    pfv_denoiser *h_ = nullptr;
};
// packed frames, frame-major ([frame][stream]), through a fresh filter in order
inline std::vector<uint8_t> frames_denoise(Context &ctx, size_t width, size_t height, const std::vector<uint8_t> &frames, const std::array<uint8_t, 3> &spatial,
                                           const std::array<uint8_t, 3> &temporal, int n_streams = 1)
{
    const size_t fb = pfv_frame_bytes((int)width, (int)height);
    if (!fb || n_streams <= 0 || frames.empty() || frames.size() % (fb * (size_t)n_streams)) throw std::invalid_argument("frames_denoise: frames must hold whole packed frames of every stream");
    std::vector<uint8_t> out(frames.size());
    ctx.check(pfv_frames_denoise(ctx.handle(), (int)width, (int)height, n_streams, (int)(frames.size() / (fb * (size_t)n_streams)), frames.data(), out.data(), spatial.data(),
                                 temporal.data()));
    return out;
}

// pfv_scene_stats (pfv_hip_ext.h, "scene-cut detection") of one pair of frames, with the score the host functions make of it
struct SceneStats : pfv_scene_stats {
    SceneStats() : pfv_scene_stats{} {}
    SceneStats(const pfv_scene_stats &s) : pfv_scene_stats(s) {}
    uint32_t score_q8() const { return pfv_scene_score_q8(this); }
};
// frame types (1 i-frame, 2 p-frame) for the frames the stats describe (pfv_scene_plan)
inline std::vector<uint8_t> scene_plan(const std::vector<SceneStats> &stats, uint32_t threshold_q8 = PFV_SCENE_THRESHOLD_DEFAULT, int min_interval = 0, int max_interval = 0)
{
    static_assert(sizeof(SceneStats) == sizeof(pfv_scene_stats), "SceneStats adds no member");
    std::vector<uint8_t> types(stats.size());
    if (pfv_scene_plan(stats.data(), (int)stats.size(), threshold_q8, min_interval, max_interval, types.data()) < 0) throw std::invalid_argument("scene_plan: bad argument");
    return types;
}
// pfv_scene_detector: the previous quarter plane and the primed flag of n_streams streams; destroy it before its context
class SceneDetector {
  public:
    SceneDetector(Context &ctx, size_t width, size_t height, int n_streams = 1, int max_clip_frames = 0) : ctx_(ctx), width_(width), height_(height), n_(n_streams)
    {
        int rc = PFV_OK;
        h_ = pfv_scene_detector_create(ctx.handle(), (int)width, (int)height, n_streams, max_clip_frames, &rc);
        if (!h_) ctx_.check(rc ? rc : PFV_ERR_BAD_ARG);
    }
    ~SceneDetector() { pfv_scene_detector_destroy(h_); }
    SceneDetector(const SceneDetector &) = delete;
    SceneDetector &operator=(const SceneDetector &) = delete;
    pfv_scene_detector *handle() const { return h_; }
    size_t frame_bytes() const { return pfv_frame_bytes((int)width_, (int)height_); }
    size_t n_blocks() const { return ((width_ >> 2) >> 3) * ((height_ >> 2) >> 3); }
    // R in quarter samples, 0 .. 7, for the runs that follow
    void set_radius(int radius) { ctx_.check(pfv_scene_detector_set_radius(h_, radius)); }
    void reset(int first_stream = 0, int n = -1) { ctx_.check(pfv_scene_detector_reset(h_, first_stream, n < 0 ? n_ - first_stream : n)); }
    // asynchronous on the context's stream, one launch group: device frames in (packed or padded, src_stride apart), n stats in device memory out
    void run_dev(int first_stream, int n, const uint8_t *src_dev, pfv_scene_stats *stats_dev, bool commit = true, int src_layout = PFV_FRAME_PACKED, size_t src_stride = 0)
    {
        ctx_.check(pfv_scene_detector_run_dev(h_, first_stream, n, src_dev, src_layout, src_stride, commit ? 1 : 0, stats_dev));
    }
    // n_frames consecutive frames of one stream, the first against the stream's state
    void run_clip_dev(int stream, int n_frames, const uint8_t *frames_dev, pfv_scene_stats *stats_dev, bool commit = true, int layout = PFV_FRAME_PACKED, size_t stride = 0)
    {
        ctx_.check(pfv_scene_detector_run_clip_dev(h_, stream, n_frames, frames_dev, layout, stride, commit ? 1 : 0, stats_dev));
    }

  private:
    Context &ctx_;
    size_t width_, height_;
    int n_;
    pfv_scene_detector *h_ = nullptr;
};
// packed frames, frame-major ([frame][stream]), through a fresh detector in order: [frame][stream] stats
inline std::vector<SceneStats> frames_scene(Context &ctx, size_t width, size_t height, const std::vector<uint8_t> &frames, int radius = PFV_SCENE_RADIUS_DEFAULT, int n_streams = 1)
{
    const size_t fb = pfv_frame_bytes((int)width, (int)height);
    if (!fb || n_streams <= 0 || frames.empty() || frames.size() % (fb * (size_t)n_streams)) throw std::invalid_argument("frames_scene: frames must hold whole packed frames of every stream");
    const size_t n_frames = frames.size() / (fb * (size_t)n_streams);
    std::vector<SceneStats> out(n_frames * (size_t)n_streams);
    ctx.check(pfv_frames_scene(ctx.handle(), (int)width, (int)height, n_streams, (int)n_frames, frames.data(), radius, out.data()));
    return out;
}

// motion search of an encoder session and of the stream encoders over it (pfv_*_set_motion_search): FourStep is the reference's search
enum class MotionSearch { FourStep = PFV_SEARCH_FOURSTEP, Full = PFV_SEARCH_FULL, Hier = PFV_SEARCH_HIER };

// The hot-path half of enc::Encoder for n streams (pfv_enc_session): packed frames of all streams in, the macroblock arrays out.
class EncoderSession {
  public:
    EncoderSession(Context &ctx, size_t width, size_t height, int quality, int n_streams = 1) : ctx_(ctx), n_(n_streams)
    {
        ctx_.check(pfv_enc_session_create(ctx.handle(), (int)width, (int)height, quality, n_streams, &h_));
        blocks_ = (size_t)pfv_total_blocks((int)width, (int)height);
        frame_bytes_ = pfv_frame_bytes((int)width, (int)height);
    }
    ~EncoderSession() { pfv_enc_session_destroy(h_); }
    EncoderSession(const EncoderSession &) = delete;
    EncoderSession &operator=(const EncoderSession &) = delete;
    pfv_enc_session *handle() const { return h_; }
    size_t total_blocks() const { return blocks_; }
    // the search of the p-frame launches that follow; radius 1 .. 15 for Full, even 2 .. 62 for Hier, ignored for FourStep
    void set_motion_search(MotionSearch mode, int radius = 0) { ctx_.check(pfv_enc_session_set_motion_search(h_, (int)mode, radius)); }
    std::pair<MotionSearch, int> motion_search() const
    {
        int m = 0, r = 0;
        ctx_.check(pfv_enc_session_get_motion_search(h_, &m, &r));
        return {(MotionSearch)m, r};
    }
    // the coarse level's vectors of the last p-frame launch, which was a Hier one: [stream][macroblock][2], half-resolution pixels
    std::vector<int8_t> coarse_vectors() const
    {
        std::vector<int8_t> out(blocks_ * (size_t)n_ * 2);
        ctx_.check(pfv_enc_session_coarse_vectors(h_, out.data(), out.size()));
        return out;
    }
    struct PFrame {
        std::vector<int8_t> mv;          // [stream][macroblock][2]
        std::vector<uint8_t> has_coef;   // [stream][macroblock]
        std::vector<int16_t> coef;       // [stream][macroblock][256]
    };
    std::vector<int16_t> encode_iframe(const std::vector<uint8_t> &frames)
    {
        check_frames(frames);
        std::vector<int16_t> coef(blocks_ * (size_t)n_ * 256);
        ctx_.check(pfv_enc_iframe(h_, frames.data(), coef.data()));
        return coef;
    }
    PFrame encode_pframe(const std::vector<uint8_t> &frames)
    {
        check_frames(frames);
        PFrame p;
        p.mv.resize(blocks_ * (size_t)n_ * 2);
        p.has_coef.resize(blocks_ * (size_t)n_);
        p.coef.resize(blocks_ * (size_t)n_ * 256);
        ctx_.check(pfv_enc_pframe(h_, frames.data(), p.mv.data(), p.has_coef.data(), p.coef.data()));
        return p;
    }

  private:
    void check_frames(const std::vector<uint8_t> &frames) const
    {
        if (frames.size() != frame_bytes_ * (size_t)n_) throw std::invalid_argument("EncoderSession: frames must hold one packed frame per stream");
    }
    Context &ctx_;
    int n_;
    size_t blocks_ = 0, frame_bytes_ = 0;
    pfv_enc_session *h_ = nullptr;
};

class Encoder {
  public:
    Encoder(std::ostream &writer, size_t width, size_t height, uint32_t framerate, int quality, Context &ctx)
        : ctx_(ctx), out_(writer), width_(width), height_(height)
    {
        ctx_.check(pfv_encoder_create(ctx.handle(), (int)width, (int)height, (int)framerate, quality, &h_));
        flush();   // the header (src/enc.rs:70)
    }
    // a quality ladder: 1..11 qualities in 0..10, strictly ascending (towards coarser quantisers); the header carries every rung's tables
    Encoder(std::ostream &writer, size_t width, size_t height, uint32_t framerate, const std::vector<int> &qualities, Context &ctx)
        : ctx_(ctx), out_(writer), width_(width), height_(height)
    {
        ctx_.check(pfv_encoder_create_ladder(ctx.handle(), (int)width, (int)height, (int)framerate, qualities.data(), (int)qualities.size(), &h_));
        flush();
    }
    ~Encoder()   // impl Drop (src/enc.rs:28-34): finish if the caller did not
    {
        if (h_) {
            if (!finished_ && pfv_encoder_finish(h_) == PFV_OK) {
                try { flush(); } catch (...) {}
            }
            pfv_encoder_destroy(h_);
        }
    }
    Encoder(const Encoder &) = delete;
    Encoder &operator=(const Encoder &) = delete;

    void encode_iframe(const VideoFrame &f)   // src/enc.rs:75-123
    {
        check_frame(f);
        ctx_.check(pfv_encoder_encode_iframe(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data()));
        flush();
    }
    void encode_pframe(const VideoFrame &f)   // src/enc.rs:125-173
    {
        check_frame(f);
        ctx_.check(pfv_encoder_encode_pframe(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data()));
        flush();
    }
    void encode_dropframe()                   // src/enc.rs:175-180
    {
        ctx_.check(pfv_encoder_encode_dropframe(h_));
        flush();
    }
    void finish()                             // src/enc.rs:182-188
    {
        ctx_.check(pfv_encoder_finish(h_));
        finished_ = true;
        flush();
    }
    // every frame as one tight picture in `format` instead of three planes: encode_iframe_rgb / encode_pframe_rgb / encode_frame_rgb then take
    // the place of the VideoFrame methods, which throw while the switch is on (the C ABI's probe calls take the picture as y with u = v = NULL)
    void set_input_rgb(bool on, PixelFormat format = PixelFormat::Rgb8, ChromaMode chroma = ChromaMode::Point)
    {
        ctx_.check(pfv_encoder_set_input_rgb(h_, on ? 1 : 0, (int)format, (int)chroma));
        rgb_bytes_ = on ? rgb_row_bytes(in_w_, format) * in_h_ : 0;
    }
    // frames -- under set_input_rgb pictures -- of src_width x src_height, resized on the device to the encoder's size; src_width 0: off
    void set_input_size(size_t src_width, size_t src_height, ScaleKind kind = ScaleKind::Bicubic)
    {
        ctx_.check(pfv_encoder_set_input_size(h_, (int)src_width, (int)src_height, (int)kind));
        const size_t bpp = rgb_bytes_ / (in_w_ * in_h_);
        in_w_ = src_width ? src_width : width_;
        in_h_ = src_width ? src_height : height_;
        rgb_bytes_ = bpp * in_w_ * in_h_;
    }
    // the noise filter as the last input stage (behind set_input_rgb and set_input_size): strengths per plane, 0 .. 16; encode_* commit its
    // state, probe_* do not
    void set_denoise(bool on, const std::array<uint8_t, 3> &spatial = {0, 0, 0}, const std::array<uint8_t, 3> &temporal = {0, 0, 0})
    {
        ctx_.check(pfv_encoder_set_denoise(h_, on ? 1 : 0, spatial.data(), temporal.data()));
    }
    void encode_iframe_rgb(const std::vector<uint8_t> &picture)
    {
        check_picture(picture);
        ctx_.check(pfv_encoder_encode_iframe(h_, picture.data(), nullptr, nullptr));
        flush();
    }
    void encode_pframe_rgb(const std::vector<uint8_t> &picture)
    {
        check_picture(picture);
        ctx_.check(pfv_encoder_encode_pframe(h_, picture.data(), nullptr, nullptr));
        flush();
    }
    int encode_frame_rgb(const std::vector<uint8_t> &picture)   // -> 1 i-frame, 2 p-frame, 3 drop frame (pfv_encoder_encode_frame)
    {
        check_picture(picture);
        int type = 0;
        ctx_.check(pfv_encoder_encode_frame(h_, picture.data(), nullptr, nullptr, &type));
        flush();
        return type;
    }
    // packet payloads from the device entropy stage (default) or the host serialisers: same bytes
    void set_device_entropy(bool on) { ctx_.check(pfv_encoder_set_device_entropy(h_, on ? 1 : 0)); }
    // on: every encode_* call also measures its frame against the reconstruction it leaves behind (last_report); same bytes
    void set_frame_report(bool on) { ctx_.check(pfv_encoder_set_frame_report(h_, on ? 1 : 0)); }
    // on: every encode_* call also measures the structural similarity of the same pair of frames (last_ssim); a switch of its own; same bytes
    void set_frame_ssim(bool on) { ctx_.check(pfv_encoder_set_frame_ssim(h_, on ? 1 : 0)); }
    // quality ladder: the rung of the frames that follow / of the last frame written (before the first frame: the current rung)
    void set_rung(int rung) { ctx_.check(pfv_encoder_set_rung(h_, rung)); }
    // the search of the p-frames that follow; Full and Hier exclude the p-frame probe, the p-frame floors and encode_frame
    void set_motion_search(MotionSearch mode, int radius = 0) { ctx_.check(pfv_encoder_set_motion_search(h_, (int)mode, radius)); }
    int rung() const { return pfv_encoder_rung(h_); }
    int n_rungs() const { return pfv_encoder_rungs(h_); }
    // byte budget per p-frame payload, 0 = off (pfv_encoder_set_rate)
    void set_rate(uint32_t pframe_budget) { ctx_.check(pfv_encoder_set_rate(h_, pframe_budget)); }
    // payload bytes of `f` as an i-frame at every rung (0xffffffff: not encodable there); the stream, the reference and the rung stay as they are
    std::vector<uint32_t> probe_iframe(const VideoFrame &f) const
    {
        check_frame(f);
        std::vector<uint32_t> sizes((size_t)n_rungs());
        ctx_.check(pfv_encoder_probe_iframe(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data(), sizes.data()));
        return sizes;
    }
    // byte budget per i-frame payload, 0 = off: encode_iframe takes the finest rung whose probed payload fits, the coarsest if none does
    void set_iframe_budget(uint32_t iframe_budget) { ctx_.check(pfv_encoder_set_iframe_budget(h_, iframe_budget)); }
    // ... and the squared error per plane at every rung, sse[3 * r + plane], from the same read of the frame (pfv_encoder_probe_iframe_rd)
    std::vector<uint32_t> probe_iframe_rd(const VideoFrame &f, std::vector<uint64_t> &sse) const
    {
        check_frame(f);
        std::vector<uint32_t> sizes((size_t)n_rungs());
        sse.assign(3 * sizes.size(), 0);
        ctx_.check(pfv_encoder_probe_iframe_rd(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data(), sizes.data(), sse.data()));
        return sizes;
    }
    // PSNR-YUV floor per i-frame in dB, 0 = off: of the rungs within the i-frame budget that reach it the one with the fewest bytes, else the
    // one with the smallest squared error (pfv_encoder_set_iframe_quality_floor)
    void set_iframe_quality_floor(double min_psnr_yuv) { ctx_.check(pfv_encoder_set_iframe_quality_floor(h_, min_psnr_yuv)); }
    // payload bytes of `f` as a p-frame against the encoder's reference at every rung; nothing changes.  Error(PFV_ERR_STATE) when poisoned or finished
    std::vector<uint32_t> probe_pframe(const VideoFrame &f) const
    {
        check_frame(f);
        std::vector<uint32_t> sizes((size_t)n_rungs());
        ctx_.check(pfv_encoder_probe_pframe(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data(), sizes.data()));
        return sizes;
    }
    // ... and the squared error per plane at every rung, sse[3 * r + plane], from the same search and transform (pfv_encoder_probe_pframe_rd)
    std::vector<uint32_t> probe_pframe_rd(const VideoFrame &f, std::vector<uint64_t> &sse) const
    {
        check_frame(f);
        std::vector<uint32_t> sizes((size_t)n_rungs());
        sse.assign(3 * sizes.size(), 0);
        ctx_.check(pfv_encoder_probe_pframe_rd(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data(), sizes.data(), sse.data()));
        return sizes;
    }
    // PSNR-YUV floor per p-frame in dB, 0 = off: of the rungs within the set_rate budget (a hard cap here) that reach it the one with the fewest
    // bytes, else the one with the smallest squared error; encode_frame then weighs the p-frame against the i-frame by the same measure
    // (pfv_encoder_set_pframe_quality_floor)
    void set_pframe_quality_floor(double min_psnr_yuv) { ctx_.check(pfv_encoder_set_pframe_quality_floor(h_, min_psnr_yuv)); }
    // ... and the SSIM sums per plane at every rung, q24[3 * r + plane], as pfv_frame_ssim.q24 of a frame written at that rung
    // (pfv_encoder_probe_iframe_ssim / pfv_encoder_probe_pframe_ssim)
    std::vector<uint32_t> probe_iframe_ssim(const VideoFrame &f, std::vector<uint64_t> &sse, std::vector<int64_t> &q24) const
    {
        check_frame(f);
        std::vector<uint32_t> sizes((size_t)n_rungs());
        sse.assign(3 * sizes.size(), 0);
        q24.assign(3 * sizes.size(), 0);
        ctx_.check(pfv_encoder_probe_iframe_ssim(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data(), sizes.data(), sse.data(), q24.data()));
        return sizes;
    }
    std::vector<uint32_t> probe_pframe_ssim(const VideoFrame &f, std::vector<uint64_t> &sse, std::vector<int64_t> &q24) const
    {
        check_frame(f);
        std::vector<uint32_t> sizes((size_t)n_rungs());
        sse.assign(3 * sizes.size(), 0);
        q24.assign(3 * sizes.size(), 0);
        ctx_.check(pfv_encoder_probe_pframe_ssim(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data(), sizes.data(), sse.data(), q24.data()));
        return sizes;
    }
    // floors on the frame's mean SSIM, 0 = off, (0, 1]: of the rungs within the budget that reach this floor and the PSNR floor the one with
    // the fewest bytes, else the one with the largest SSIM (pfv_encoder_set_iframe_ssim_floor / pfv_encoder_set_pframe_ssim_floor)
    void set_iframe_ssim_floor(double min_ssim) { ctx_.check(pfv_encoder_set_iframe_ssim_floor(h_, min_ssim)); }
    void set_pframe_ssim_floor(double min_ssim) { ctx_.check(pfv_encoder_set_pframe_ssim_floor(h_, min_ssim)); }
    // on, with a set_rate budget and more than one rung: encode_pframe takes the finest rung whose probed payload fits, the coarsest if none does
    void set_pframe_probe(bool on) { ctx_.check(pfv_encoder_set_pframe_probe(h_, on ? 1 : 0)); }
    // encode_frame forces an i-frame once max_interval frames (drop frames included) have followed the last one; 0 = never
    void set_gop(int max_interval) { ctx_.check(pfv_encoder_set_gop(h_, max_interval)); }
    // scene-cut detection on the staged frame of every encode_* (committed) and probe_* (uncommitted) call; encode_frame then writes an i-frame
    // where the score reaches threshold_q8 and min_interval frames have followed the last one, in every search mode (pfv_encoder_set_scene_cut)
    void set_scene_cut(bool on, uint32_t threshold_q8 = PFV_SCENE_THRESHOLD_DEFAULT, int radius = PFV_SCENE_RADIUS_DEFAULT, int min_interval = 0)
    {
        ctx_.check(pfv_encoder_set_scene_cut(h_, on ? 1 : 0, threshold_q8, radius, min_interval));
    }
    // the stats of the last call that measured a frame; pfv::Error(PFV_ERR_STATE) when the switch is off or nothing has been measured
    SceneStats last_scene() const
    {
        pfv_scene_stats s;
        ctx_.check(pfv_encoder_last_scene(h_, &s));
        return SceneStats(s);
    }
    // the frame's type chosen by the probes (pfv_encoder_encode_frame) -> 1 i-frame, 2 p-frame, 3 drop frame
    int encode_frame(const VideoFrame &f)
    {
        check_frame(f);
        int type = 0;
        ctx_.check(pfv_encoder_encode_frame(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data(), &type));
        flush();
        return type;
    }
    // of the last encode_* call; Error(PFV_ERR_STATE) when reports are off, nothing has been encoded yet or that call failed
    FrameReport last_report() const
    {
        pfv_frame_report r;
        ctx_.check(pfv_encoder_frame_report(h_, &r));
        FrameReport out;
        out.type = (int)r.type;
        out.packet_bytes = r.packet_bytes;
        for (int i = 0; i < 3; i++) { out.sse[i] = r.sse[i]; out.psnr[i] = r.psnr[i]; }
        out.psnr_yuv = r.psnr_yuv;
        return out;
    }
    // of the last encode_* call; Error(PFV_ERR_STATE) when set_frame_ssim is off, nothing has been encoded yet or that call failed
    FrameSsim last_ssim() const
    {
        pfv_frame_ssim r;
        ctx_.check(pfv_encoder_frame_ssim(h_, &r));
        FrameSsim out;
        for (int i = 0; i < 3; i++) { out.q24[i] = r.q24[i]; out.windows[i] = r.windows[i]; out.ssim[i] = r.ssim[i]; }
        out.ssim_all = r.ssim_all;
        return out;
    }

  private:
    void check_picture(const std::vector<uint8_t> &picture) const
    {
        if (!rgb_bytes_) throw std::logic_error("Encoder: set_input_rgb(true) first");
        if (picture.size() != rgb_bytes_) throw std::invalid_argument("Encoder: the picture is not one tight picture of the encoder's size and format");
    }
    void check_frame(const VideoFrame &f) const   // the asserts of src/enc.rs:76-80
    {
        if (rgb_bytes_) throw std::logic_error("Encoder: the encoder takes RGB pictures (set_input_rgb): use the _rgb methods");
        if (f.width != in_w_ || f.height != in_h_ || f.plane_y.pixels.size() != in_w_ * in_h_ ||
            f.plane_u.pixels.size() != (in_w_ / 2) * (in_h_ / 2) || f.plane_v.pixels.size() != (in_w_ / 2) * (in_h_ / 2))
            throw std::invalid_argument("Encoder: frame geometry does not match the encoder (src/enc.rs:76-79)");
    }
    void flush()
    {
        const uint8_t *data = nullptr;
        size_t len = 0;
        ctx_.check(pfv_encoder_drain(h_, &data, &len));   // hands the pending bytes over; the library keeps nothing
        if (len) out_.write(reinterpret_cast<const char *>(data), (std::streamsize)len);
        if (!out_) throw Error(PFV_ERR_IO, "Encoder: the writer failed (the reference propagates io::Error, src/enc.rs:190-235)");
    }
    Context &ctx_;
    std::ostream &out_;
    size_t width_, height_;
    size_t in_w_ = width_, in_h_ = height_;   // the size of what the encode calls take: set_input_size's, else the encoder's
    size_t rgb_bytes_ = 0;          // set_input_rgb: the size of one picture; 0 while the switch is off
    bool finished_ = false;
    pfv_encoder *h_ = nullptr;
};

// src/dec.rs:15-224
class Decoder {
  public:
    using OnVideo = std::function<void(const VideoFrame &)>;
    using OnPicture = std::function<void(const std::vector<uint8_t> &pixels, uint32_t width, uint32_t height)>;   // one tight picture (set_output_rgb)

    Decoder(std::istream &reader, Context &ctx)
        : ctx_(ctx), data_((std::istreambuf_iterator<char>(reader)), std::istreambuf_iterator<char>())
    {
        int rc = pfv_decoder_create(ctx.handle(), reinterpret_cast<const uint8_t *>(data_.data()), data_.size(), &h_);
        if (rc != PFV_OK) ctx_.check(rc);   // DecodeError::{FormatError, VersionError, IOError} (src/dec.rs:30-35)
        frame_ = VideoFrame((size_t)width(), (size_t)height());
    }
    ~Decoder() { pfv_decoder_destroy(h_); }
    Decoder(const Decoder &) = delete;
    Decoder &operator=(const Decoder &) = delete;

    uint32_t width() const { return (uint32_t)pfv_decoder_width(h_); }          // src/dec.rs:136-138
    uint32_t height() const { return (uint32_t)pfv_decoder_height(h_); }        // :140-142
    uint32_t framerate() const { return (uint32_t)pfv_decoder_framerate(h_); }  // :144-146
    void reset() { ctx_.check(pfv_decoder_reset(h_)); }                         // :148-152
    void set_lookahead(int n_threads) { ctx_.check(pfv_decoder_set_lookahead(h_, n_threads)); }
    // out-of-loop deblocking of the frames onvideo receives: Auto takes the strengths from the q-tables each packet names, Fixed the ones given;
    // what the next p-frame predicts from is untouched
    void set_deblock(Deblock mode, const std::array<uint8_t, 3> &strength = {0, 0, 0}) { ctx_.check(pfv_decoder_set_deblock(h_, (int)mode, strength.data())); }

    // every decoded frame as one tight picture in `format` instead of three planes: advance_frame_rgb / advance_delta_rgb then take the place of
    // advance_frame / advance_delta (frames, order and errors are the same)
    void set_output_rgb(bool on, PixelFormat format = PixelFormat::Rgb8)
    {
        ctx_.check(pfv_decoder_set_output_rgb(h_, on ? 1 : 0, (int)format));
        rgb_bytes_ = on ? rgb_row_bytes(out_w_ ? out_w_ : width(), format) * (out_w_ ? out_h_ : height()) : 0;
    }
    // every frame -- under set_output_rgb every picture -- resized on the device to out_width x out_height; out_width 0: off.  width() and
    // height() keep the stream's size; the callback's frame carries its own
    void set_output_size(size_t out_width, size_t out_height, ScaleKind kind = ScaleKind::Bicubic)
    {
        ctx_.check(pfv_decoder_set_output_size(h_, (int)out_width, (int)out_height, (int)kind));
        const size_t w0 = out_w_ ? out_w_ : width(), h0 = out_w_ ? out_h_ : height(), bpp = rgb_bytes_ / (w0 * h0);
        out_w_ = out_width;
        out_h_ = out_width ? out_height : 0;
        rgb_bytes_ = bpp * (out_w_ ? out_w_ * out_h_ : (size_t)width() * height());
    }
    bool advance_frame_rgb(const OnPicture &onpicture)
    {
        if (!rgb_bytes_) throw std::logic_error("Decoder::advance_frame_rgb: set_output_rgb(true) first");
        pic_cb_ = &onpicture;
        return result(pfv_decoder_advance_frame(h_, &Decoder::trampoline_rgb, this));
    }
    bool advance_delta_rgb(double delta, const OnPicture &onpicture)
    {
        if (!rgb_bytes_) throw std::logic_error("Decoder::advance_delta_rgb: set_output_rgb(true) first");
        pic_cb_ = &onpicture;
        return result(pfv_decoder_advance_delta(h_, delta, &Decoder::trampoline_rgb, this));
    }

    // false at the end of the stream (Ok(false)), true otherwise; onvideo is called for every decoded frame
    bool advance_delta(double delta, const OnVideo &onvideo)                    // src/dec.rs:154-167
    {
        if (rgb_bytes_) throw std::logic_error("Decoder::advance_delta: the callback gets RGB pictures (set_output_rgb): use advance_delta_rgb");
        cb_ = &onvideo;
        return result(pfv_decoder_advance_delta(h_, delta, &Decoder::trampoline, this));
    }
    bool advance_frame(const OnVideo &onvideo)                                  // src/dec.rs:169-224
    {
        if (rgb_bytes_) throw std::logic_error("Decoder::advance_frame: the callback gets RGB pictures (set_output_rgb): use advance_frame_rgb");
        cb_ = &onvideo;
        return result(pfv_decoder_advance_frame(h_, &Decoder::trampoline, this));
    }

  private:
    bool result(int rc)
    {
        cb_ = nullptr;
        pic_cb_ = nullptr;
        if (rc < 0) ctx_.check(rc);
        return rc == 1;
    }
    static void trampoline_rgb(void *user, const uint8_t *y, const uint8_t *, const uint8_t *, int w, int h)
    {
        Decoder *d = static_cast<Decoder *>(user);
        d->picture_.assign(y, y + d->rgb_bytes_);
        if (d->pic_cb_ && *d->pic_cb_) (*d->pic_cb_)(d->picture_, (uint32_t)w, (uint32_t)h);
    }
    static void trampoline(void *user, const uint8_t *y, const uint8_t *u, const uint8_t *v, int w, int h)
    {
        Decoder *d = static_cast<Decoder *>(user);
        const size_t ny = (size_t)w * h, nc = (size_t)(w / 2) * (h / 2);
        if (d->frame_.width != (size_t)w || d->frame_.height != (size_t)h) d->frame_ = VideoFrame((size_t)w, (size_t)h);   // set_output_size
        d->frame_.plane_y.pixels.assign(y, y + ny);
        d->frame_.plane_u.pixels.assign(u, u + nc);
        d->frame_.plane_v.pixels.assign(v, v + nc);
        if (d->cb_ && *d->cb_) (*d->cb_)(d->frame_);
    }
    Context &ctx_;
    std::string data_;              // the whole stream: the native decoder reads from it for its lifetime
    pfv_decoder *h_ = nullptr;
    VideoFrame frame_;              // retframe (src/dec.rs:22)
    const OnVideo *cb_ = nullptr;
    std::vector<uint8_t> picture_;  // set_output_rgb: the picture the callback sees
    size_t rgb_bytes_ = 0;          // its size; 0 while the switch is off
    size_t out_w_ = 0, out_h_ = 0;  // set_output_size; 0 while the switch is off
    const OnPicture *pic_cb_ = nullptr;
};

// Encoder with the GOPs of the stream batched per launch (pfv_gop_encoder, pfv_hip.h): same calls, same .pfv bytes; a packet reaches the
// writer when its batch of max_gops groups is complete, on flush() or on finish().  Packets are written segment by segment from where
// they lie (pfv_gop_encoder_drain_iov): no copy on the way to the writer.
class GopEncoder {
  public:
    GopEncoder(std::ostream &writer, size_t width, size_t height, uint32_t framerate, int quality, Context &ctx, int max_gops = 8, int max_gop_frames = 15,
               size_t payload_budget = 0)
        : ctx_(ctx), out_(writer), width_(width), height_(height)
    {
        ctx_.check(pfv_gop_encoder_create(ctx.handle(), (int)width, (int)height, (int)framerate, quality, max_gops, max_gop_frames, payload_budget, &h_));
        drain();   // the header (src/enc.rs:70)
    }
    ~GopEncoder()   // impl Drop (src/enc.rs:28-34)
    {
        if (h_) {
            if (!finished_ && pfv_gop_encoder_finish(h_) == PFV_OK) {
                try { drain(); } catch (...) {}
            }
            pfv_gop_encoder_destroy(h_);
        }
    }
    GopEncoder(const GopEncoder &) = delete;
    GopEncoder &operator=(const GopEncoder &) = delete;
    void encode_iframe(const VideoFrame &f)   // src/enc.rs:75-123
    {
        check_frame(f);
        ctx_.check(pfv_gop_encoder_encode_iframe(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data()));
        drain();
    }
    void encode_pframe(const VideoFrame &f)   // src/enc.rs:125-173
    {
        check_frame(f);
        ctx_.check(pfv_gop_encoder_encode_pframe(h_, f.plane_y.pixels.data(), f.plane_u.pixels.data(), f.plane_v.pixels.data()));
        drain();
    }
    // device frames are read where they lie instead of being copied into the batch; the caller keeps each one valid and unchanged until its
    // packet has reached the writer (or flush() / finish() returned)
    void set_frames_by_reference(bool on) { ctx_.check(pfv_gop_encoder_set_frames_by_reference(h_, on ? 1 : 0)); }
    // the search of the batches submitted from now on; throws (PFV_ERR_STATE) while a batch is in flight
    void set_motion_search(MotionSearch mode, int radius = 0) { ctx_.check(pfv_gop_encoder_set_motion_search(h_, (int)mode, radius)); }
    // a packed frame (Y | U | V) that already lies in device memory: nothing crosses PCIe on the way in.  Stream-ordered on the context's
    // stream like every *_dev call: no host wait, the frame may only be overwritten by work enqueued on that stream afterwards
    void encode_iframe_device(const uint8_t *frame_dev)
    {
        ctx_.check(pfv_gop_encoder_encode_iframe_dev(h_, frame_dev));
        drain();
    }
    void encode_pframe_device(const uint8_t *frame_dev)
    {
        ctx_.check(pfv_gop_encoder_encode_pframe_dev(h_, frame_dev));
        drain();
    }
    void encode_dropframe() { ctx_.check(pfv_gop_encoder_encode_dropframe(h_)); }   // src/enc.rs:175-180
    void flush()                              // every frame handed over so far becomes packets at the writer now
    {
        ctx_.check(pfv_gop_encoder_flush(h_));
        drain();
    }
    void finish()                             // src/enc.rs:182-188
    {
        ctx_.check(pfv_gop_encoder_finish(h_));
        finished_ = true;
        drain();
    }
    long batches() const { return pfv_gop_encoder_batches(h_); }

  private:
    void check_frame(const VideoFrame &f) const   // the asserts of src/enc.rs:76-80
    {
        if (f.width != width_ || f.height != height_ || f.plane_y.pixels.size() != width_ * height_ ||
            f.plane_u.pixels.size() != (width_ / 2) * (height_ / 2) || f.plane_v.pixels.size() != (width_ / 2) * (height_ / 2))
            throw std::invalid_argument("GopEncoder: frame geometry does not match the encoder (src/enc.rs:76-79)");
    }
    void drain()
    {
        const pfv_iovec *iov = nullptr;
        size_t n = 0;
        ctx_.check(pfv_gop_encoder_drain_iov(h_, &iov, &n));
        for (size_t i = 0; i < n; i++) out_.write(reinterpret_cast<const char *>(iov[i].data), (std::streamsize)iov[i].len);
        if (!out_) throw Error(PFV_ERR_IO, "GopEncoder: the writer failed (the reference propagates io::Error, src/enc.rs:190-235)");
    }
    Context &ctx_;
    std::ostream &out_;
    size_t width_, height_;
    bool finished_ = false;
    pfv_gop_encoder *h_ = nullptr;
};

// Decoder with the GOPs of the stream batched per launch (pfv_gop_decoder): the frames, their order and the result of every call are
// those of pfv::Decoder; n_threads packet parsers work beside the caller.
class GopDecoder {
  public:
    using OnVideo = std::function<void(const VideoFrame &)>;
    GopDecoder(std::istream &reader, Context &ctx, int max_gops = 8, int max_gop_frames = 15, int n_threads = 4)
        : ctx_(ctx), data_((std::istreambuf_iterator<char>(reader)), std::istreambuf_iterator<char>())
    {
        int rc = pfv_gop_decoder_create(ctx.handle(), reinterpret_cast<const uint8_t *>(data_.data()), data_.size(), max_gops, max_gop_frames, n_threads, &h_);
        if (rc != PFV_OK) ctx_.check(rc);
        frame_ = VideoFrame((size_t)width(), (size_t)height());
    }
    ~GopDecoder() { pfv_gop_decoder_destroy(h_); }
    GopDecoder(const GopDecoder &) = delete;
    GopDecoder &operator=(const GopDecoder &) = delete;
    uint32_t width() const { return (uint32_t)pfv_gop_decoder_width(h_); }
    uint32_t height() const { return (uint32_t)pfv_gop_decoder_height(h_); }
    uint32_t framerate() const { return (uint32_t)pfv_gop_decoder_framerate(h_); }
    void reset() { ctx_.check(pfv_gop_decoder_reset(h_)); }
    // With set_output_device(true) the frames live in device memory: the host-frame callbacks below would read device pointers, so they
    // refuse (use the *_device forms).
    bool advance_delta(double delta, const OnVideo &onvideo)
    {
        if (device_out_) throw std::logic_error("GopDecoder::advance_delta: frames stay in device memory (set_output_device): use advance_delta_device");
        cb_ = &onvideo;
        return result(pfv_gop_decoder_advance_delta(h_, delta, &GopDecoder::trampoline, this));
    }
    bool advance_frame(const OnVideo &onvideo)
    {
        if (device_out_) throw std::logic_error("GopDecoder::advance_frame: frames stay in device memory (set_output_device): use advance_frame_device");
        cb_ = &onvideo;
        return result(pfv_gop_decoder_advance_frame(h_, &GopDecoder::trampoline, this));
    }
    // frames left in device memory (pfv_gop_decoder_set_output_device): the consumer gets the three planes' DEVICE addresses, valid until
    // the call that starts the next batch -- for consumers on the GPU; no frame crosses PCIe
    using OnVideoDevice = std::function<void(const uint8_t *y, const uint8_t *u, const uint8_t *v, uint32_t width, uint32_t height)>;
    void set_output_device(bool on) { ctx_.check(pfv_gop_decoder_set_output_device(h_, on ? 1 : 0)); device_out_ = on; }
    bool advance_frame_device(const OnVideoDevice &onvideo)
    {
        if (!device_out_) throw std::logic_error("GopDecoder::advance_frame_device: set_output_device(true) first");
        dcb_ = &onvideo;
        const int rc = pfv_gop_decoder_advance_frame(h_, &GopDecoder::trampoline_device, this);
        dcb_ = nullptr;
        if (rc < 0) ctx_.check(rc);
        return rc == 1;
    }
    bool advance_delta_device(double delta, const OnVideoDevice &onvideo)       // Decoder::advance_delta (src/dec.rs:154-167), frames in device memory
    {
        if (!device_out_) throw std::logic_error("GopDecoder::advance_delta_device: set_output_device(true) first");
        dcb_ = &onvideo;
        const int rc = pfv_gop_decoder_advance_delta(h_, delta, &GopDecoder::trampoline_device, this);
        dcb_ = nullptr;
        if (rc < 0) ctx_.check(rc);
        return rc == 1;
    }

  private:
    static void trampoline_device(void *user, const uint8_t *y, const uint8_t *u, const uint8_t *v, int w, int h)
    {
        GopDecoder *d = static_cast<GopDecoder *>(user);
        if (d->dcb_ && *d->dcb_) (*d->dcb_)(y, u, v, (uint32_t)w, (uint32_t)h);
    }
    bool result(int rc)
    {
        cb_ = nullptr;
        if (rc < 0) ctx_.check(rc);
        return rc == 1;
    }
    static void trampoline(void *user, const uint8_t *y, const uint8_t *u, const uint8_t *v, int w, int h)
    {
        GopDecoder *d = static_cast<GopDecoder *>(user);
        const size_t ny = (size_t)w * h, nc = (size_t)(w / 2) * (h / 2);
        d->frame_.plane_y.pixels.assign(y, y + ny);
        d->frame_.plane_u.pixels.assign(u, u + nc);
        d->frame_.plane_v.pixels.assign(v, v + nc);
        if (d->cb_ && *d->cb_) (*d->cb_)(d->frame_);
    }
    Context &ctx_;
    std::string data_;
    pfv_gop_decoder *h_ = nullptr;
    VideoFrame frame_;
    const OnVideo *cb_ = nullptr;
    const OnVideoDevice *dcb_ = nullptr;
    bool device_out_ = false;
};

// n Encoders of one geometry stepped together (pfv_batch_encoder): every writer receives exactly the bytes an Encoder of
// its own would have written (src/enc.rs:12-188); packets arrive one step late, finish() / the destructor flush.
class BatchEncoder {
  public:
    BatchEncoder(std::vector<std::ostream *> writers, size_t width, size_t height, uint32_t framerate, int quality, Context &ctx)
        : ctx_(ctx), writers_(std::move(writers))
    {
        ctx_.check(pfv_batch_encoder_create(ctx.handle(), (int)width, (int)height, (int)framerate, quality, (int)writers_.size(), &on_write, this, &h_));
        frame_bytes_ = pfv_frame_bytes((int)width, (int)height);
    }
    ~BatchEncoder()
    {
        if (h_) {
            if (!finished_) {
                try { finish(); } catch (...) {}
            }
            pfv_batch_encoder_destroy(h_);
        }
    }
    BatchEncoder(const BatchEncoder &) = delete;
    BatchEncoder &operator=(const BatchEncoder &) = delete;
    size_t frame_bytes() const { return frame_bytes_; }
    // page-locked [n][frame_bytes] array to fill for the next encode call (packed Y|U|V per stream)
    uint8_t *frames() { return pfv_batch_encoder_frames(h_); }
    void encode_iframes() { done(pfv_batch_encoder_encode(h_, 0, nullptr)); }
    void encode_pframes() { done(pfv_batch_encoder_encode(h_, 1, nullptr)); }
    void finish()
    {
        const int rc = pfv_batch_encoder_finish(h_);
        finished_ = true;
        done(rc);
    }

  private:
    // A writer that fails (disk full, closed pipe) must not go unnoticed: the reference propagates every write error (`?`,
    // src/enc.rs:190-235).  Nothing may unwind through the C callback, so the failure is remembered, all further writes are
    // dropped (no writer receives bytes behind a hole) and the call that triggered it throws.
    static void on_write(void *user, int stream, const uint8_t *data, size_t len)
    {
        auto *self = static_cast<BatchEncoder *>(user);
        if (self->failed_stream_ >= 0) return;
        std::ostream *w = self->writers_[(size_t)stream];
        w->write(reinterpret_cast<const char *>(data), (std::streamsize)len);
        if (!*w) self->failed_stream_ = stream;
    }
    void done(int rc)
    {
        if (failed_stream_ >= 0) {
            finished_ = true;
            throw Error(PFV_ERR_IO, "BatchEncoder: writer " + std::to_string(failed_stream_) + " failed; its stream is truncated");
        }
        ctx_.check(rc);
    }
    int failed_stream_ = -1;
    Context &ctx_;
    std::vector<std::ostream *> writers_;
    size_t frame_bytes_ = 0;
    bool finished_ = false;
    pfv_batch_encoder *h_ = nullptr;
};

// n Decoders in lockstep (pfv_batch_decoder): advance_frames() -> 1 frames (page-locked [n][frame_bytes], valid until the call
// after next), 2 a step of drop frames, 0 end of the streams; errors as pfv::Error with the DecodeError codes.
class BatchDecoder {
  public:
    BatchDecoder(std::vector<std::string> streams, Context &ctx, int n_threads = 8) : ctx_(ctx), data_(std::move(streams))
    {
        std::vector<const uint8_t *> p;
        std::vector<size_t> n;
        for (const auto &s : data_) { p.push_back(reinterpret_cast<const uint8_t *>(s.data())); n.push_back(s.size()); }
        ctx_.check(pfv_batch_decoder_create(ctx.handle(), p.data(), n.data(), (int)data_.size(), n_threads, &h_));
    }
    ~BatchDecoder() { pfv_batch_decoder_destroy(h_); }
    BatchDecoder(const BatchDecoder &) = delete;
    BatchDecoder &operator=(const BatchDecoder &) = delete;
    size_t width() const { return (size_t)pfv_batch_decoder_width(h_); }
    size_t height() const { return (size_t)pfv_batch_decoder_height(h_); }
    uint32_t framerate() const { return (uint32_t)pfv_batch_decoder_framerate(h_); }
    int advance_frames(const uint8_t **frames)
    {
        const int rc = pfv_batch_decoder_advance(h_, frames);
        if (rc < 0) ctx_.check(rc);
        return rc;
    }

  private:
    Context &ctx_;
    std::vector<std::string> data_;
    pfv_batch_decoder *h_ = nullptr;
};

}  // namespace pfv
