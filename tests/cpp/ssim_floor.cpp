// The p-frame SSIM probe and SSIM floor through include/pfv_hip.hpp (pfv::Encoder::probe_pframe_ssim, set_pframe_ssim_floor).
// usage: ssim_floor run W H Q0,Q1,... RUNG MIN_SSIM in.yuv out.pfv
//   reads raw 4:2:0 frames; frame 0 is an i-frame at RUNG, every later frame is probed and then encoded as a p-frame under the floor; the stream
//   goes to a file.  Prints per p-frame one line "sizes <probed bytes per rung>", one line "sse <Y U V per rung>" and one line
//   "q24 <Y U V per rung>", then "rungs <rung of every frame>"; the Python test compares them, and the bytes, with the model's.
// usage: ssim_floor poison W H Q0,Q1,... in.yuv        (built with -DSSIM_FLOOR_SEAM against the seam build of the emulator library, two frames)
//   tests/cpp/poison_seam.h fails the payload-size download of a p-frame behind its encode kernel: prints "failed <rc>", "poisoned <rc of
//   probe_pframe_ssim>", then, behind an i-frame, "recovered <rc of probe_pframe_ssim>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "pfv_hip.hpp"

#ifdef SSIM_FLOOR_SEAM
extern int pfv_seam_fail_d2h;
#endif

static std::vector<int> ladder(const char *arg)
{
    std::vector<int> qualities;
    std::stringstream list(arg);
    std::string item;
    while (std::getline(list, item, ',')) qualities.push_back(std::atoi(item.c_str()));
    return qualities;
}

static bool read_frame(std::ifstream &in, pfv::VideoFrame &f)
{
    in.read(reinterpret_cast<char *>(f.plane_y.pixels.data()), (std::streamsize)f.plane_y.pixels.size());
    in.read(reinterpret_cast<char *>(f.plane_u.pixels.data()), (std::streamsize)f.plane_u.pixels.size());
    in.read(reinterpret_cast<char *>(f.plane_v.pixels.data()), (std::streamsize)f.plane_v.pixels.size());
    return (bool)in;
}

static int run(char **argv)
{
    const size_t w = std::strtoul(argv[2], nullptr, 10), h = std::strtoul(argv[3], nullptr, 10);
    const std::vector<int> qualities = ladder(argv[4]);
    const int rung = std::atoi(argv[5]);
    const double floor_ssim = std::strtod(argv[6], nullptr);
    pfv::Context ctx(0);
    std::ifstream in(argv[7], std::ios::binary);
    std::stringstream stream(std::ios::in | std::ios::out | std::ios::binary);
    pfv::Encoder enc(stream, w, h, 30, qualities, ctx);
    enc.set_rung(rung);
    enc.set_iframe_ssim_floor(0.0);
    enc.set_pframe_ssim_floor(floor_ssim);
    pfv::VideoFrame f(w, h);
    std::string rungs = "rungs";
    for (int t = 0; read_frame(in, f); t++) {
        if (t == 0) {
            enc.encode_iframe(f);
        } else {
            const int before = enc.rung();
            std::vector<uint64_t> sse;
            std::vector<int64_t> q24;
            const std::vector<uint32_t> sizes = enc.probe_pframe_ssim(f, sse, q24);
            if (sizes.size() != qualities.size() || sse.size() != 3 * qualities.size() || q24.size() != sse.size() || enc.rung() != before) {
                std::fprintf(stderr, "probe_pframe_ssim: %zu sizes, %zu / %zu sums, rung %d -> %d\n", sizes.size(), sse.size(), q24.size(), before, enc.rung());
                return 1;
            }
            std::string line = "sizes";
            for (uint32_t n : sizes) line += " " + std::to_string(n);
            std::printf("%s\n", line.c_str());
            line = "sse";
            for (uint64_t n : sse) line += " " + std::to_string(n);
            std::printf("%s\n", line.c_str());
            line = "q24";
            for (int64_t n : q24) line += " " + std::to_string(n);
            std::printf("%s\n", line.c_str());
            enc.encode_pframe(f);
        }
        rungs += " " + std::to_string(enc.rung());
    }
    enc.finish();
    std::printf("%s\n", rungs.c_str());
    const std::string bytes = stream.str();
    std::ofstream(argv[8], std::ios::binary).write(bytes.data(), (std::streamsize)bytes.size());
    return 0;
}

#ifdef SSIM_FLOOR_SEAM
static int poison(char **argv)
{
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    std::vector<int> q = ladder(argv[4]);
    const size_t ny = (size_t)w * h, nc = (size_t)(w / 2) * (h / 2), fb = ny + 2 * nc;
    std::vector<uint8_t> clip(2 * fb);
    if (!std::ifstream(argv[5], std::ios::binary).read(reinterpret_cast<char *>(clip.data()), (std::streamsize)clip.size())) return 2;
    auto Y = [&](int t) { return clip.data() + t * fb; };
    auto U = [&](int t) { return clip.data() + t * fb + ny; };
    auto V = [&](int t) { return clip.data() + t * fb + ny + nc; };
    pfv_ctx *ctx = nullptr;
    pfv_encoder *e = nullptr;
    if (pfv_ctx_create(0, &ctx) != PFV_OK || pfv_encoder_create_ladder(ctx, w, h, 30, q.data(), (int)q.size(), &e) != PFV_OK) return 1;
    if (pfv_encoder_encode_iframe(e, Y(0), U(0), V(0)) != PFV_OK) return 1;
    pfv_seam_fail_d2h = 1;                                        // the payload size of the next frame does not come down
    const int failed = pfv_encoder_encode_pframe(e, Y(1), U(1), V(1));
    if (pfv_seam_fail_d2h != 0) { std::fprintf(stderr, "the seam was not reached\n"); return 1; }
    std::printf("failed %d\n", failed);
    std::vector<uint32_t> sizes(q.size());
    std::vector<uint64_t> sse(3 * q.size());
    std::vector<int64_t> q24(3 * q.size());
    std::printf("poisoned %d\n", pfv_encoder_probe_pframe_ssim(e, Y(1), U(1), V(1), sizes.data(), sse.data(), q24.data()));
    if (pfv_encoder_encode_iframe(e, Y(1), U(1), V(1)) != PFV_OK) return 1;
    std::printf("recovered %d\n", pfv_encoder_probe_pframe_ssim(e, Y(1), U(1), V(1), sizes.data(), sse.data(), q24.data()));
    pfv_encoder_destroy(e);
    pfv_ctx_destroy(ctx);
    return 0;
}
#endif

int main(int argc, char **argv)
{
    try {
        if (argc == 9 && !std::strcmp(argv[1], "run")) return run(argv);
#ifdef SSIM_FLOOR_SEAM
        if (argc == 6 && !std::strcmp(argv[1], "poison")) return poison(argv);
#endif
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    std::fprintf(stderr, "usage: %s run W H Q0,Q1,... RUNG MIN_SSIM in.yuv out.pfv | poison W H Q0,Q1,... in.yuv\n", argv[0]);
    return 2;
}
