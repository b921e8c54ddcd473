// The i-frame rate-distortion probe and quality floor through include/pfv_hip.hpp (pfv::Encoder::probe_iframe_rd, set_iframe_quality_floor):
// reads raw 4:2:0 frames, probes every frame, encodes frame 0 and every I_PERIOD-th frame as an i-frame under the quality floor and the rest as
// p-frames under the p-frame budget, writes the stream to a file.
// usage: rd_floor W H Q0,Q1,... MIN_PSNR_YUV PFRAME_BUDGET I_PERIOD in.yuv out.pfv
// Prints per frame one line "sizes <probed bytes per rung>" and one line "sse <Y U V per rung>", then "rungs <rung of every frame>"; the
// Python test compares them, and the bytes, with the model's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: %s W H Q0,Q1,... MIN_PSNR_YUV PFRAME_BUDGET I_PERIOD in.yuv out.pfv\n", argv[0]); return 2; }
    const size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    std::vector<int> qualities;
    {
        std::stringstream list(argv[3]);
        std::string item;
        while (std::getline(list, item, ',')) qualities.push_back(std::atoi(item.c_str()));
    }
    const double floor_db = std::strtod(argv[4], nullptr);
    const uint32_t budget_p = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    const int period = std::atoi(argv[6]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[7], std::ios::binary);
        std::stringstream stream(std::ios::in | std::ios::out | std::ios::binary);
        pfv::Encoder enc(stream, w, h, 30, qualities, ctx);
        enc.set_iframe_quality_floor(floor_db);
        enc.set_rate(budget_p);
        pfv::VideoFrame f(w, h);
        std::string rungs = "rungs";
        for (int t = 0;; t++) {
            in.read(reinterpret_cast<char *>(f.plane_y.pixels.data()), (std::streamsize)f.plane_y.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_u.pixels.data()), (std::streamsize)f.plane_u.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_v.pixels.data()), (std::streamsize)f.plane_v.pixels.size());
            if (!in) break;
            const int before = enc.rung();
            std::vector<uint64_t> sse;
            const std::vector<uint32_t> sizes = enc.probe_iframe_rd(f, sse);
            if (sizes.size() != qualities.size() || sse.size() != 3 * qualities.size() || enc.rung() != before) {
                std::fprintf(stderr, "probe_iframe_rd: %zu sizes, %zu sums, rung %d -> %d\n", sizes.size(), sse.size(), before, enc.rung());
                return 1;
            }
            std::string line = "sizes";
            for (uint32_t n : sizes) line += " " + std::to_string(n);
            std::printf("%s\n", line.c_str());
            line = "sse";
            for (uint64_t n : sse) line += " " + std::to_string(n);
            std::printf("%s\n", line.c_str());
            if (t % period == 0) enc.encode_iframe(f);
            else enc.encode_pframe(f);
            rungs += " " + std::to_string(enc.rung());
        }
        enc.finish();
        std::printf("%s\n", rungs.c_str());
        const std::string bytes = stream.str();
        std::ofstream(argv[8], std::ios::binary).write(bytes.data(), (std::streamsize)bytes.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
