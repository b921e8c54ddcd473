// The i-frame size probe and byte budget through include/pfv_hip.hpp (pfv::Encoder::probe_iframe, set_iframe_budget): reads raw 4:2:0 frames,
// probes every frame, encodes frame 0 and every I_PERIOD-th frame as an i-frame under the i-frame budget and the rest as p-frames under the
// p-frame budget, writes the stream to a file.
// usage: probe_budget W H Q0,Q1,... IFRAME_BUDGET PFRAME_BUDGET I_PERIOD in.yuv out.pfv
// Prints one line "sizes <probed bytes per rung>" per frame, then "rungs <rung of every frame>"; the Python test compares them, and the
// bytes, with the model's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: %s W H Q0,Q1,... IFRAME_BUDGET PFRAME_BUDGET I_PERIOD in.yuv out.pfv\n", argv[0]); return 2; }
    const size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    std::vector<int> qualities;
    {
        std::stringstream list(argv[3]);
        std::string item;
        while (std::getline(list, item, ',')) qualities.push_back(std::atoi(item.c_str()));
    }
    const uint32_t budget_i = (uint32_t)std::strtoul(argv[4], nullptr, 10), budget_p = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    const int period = std::atoi(argv[6]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[7], std::ios::binary);
        std::stringstream stream(std::ios::in | std::ios::out | std::ios::binary);
        pfv::Encoder enc(stream, w, h, 30, qualities, ctx);
        enc.set_iframe_budget(budget_i);
        enc.set_rate(budget_p);
        pfv::VideoFrame f(w, h);
        std::string rungs = "rungs";
        for (int t = 0;; t++) {
            in.read(reinterpret_cast<char *>(f.plane_y.pixels.data()), (std::streamsize)f.plane_y.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_u.pixels.data()), (std::streamsize)f.plane_u.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_v.pixels.data()), (std::streamsize)f.plane_v.pixels.size());
            if (!in) break;
            const int before = enc.rung();
            const std::vector<uint32_t> sizes = enc.probe_iframe(f);
            if (sizes.size() != qualities.size() || enc.rung() != before) { std::fprintf(stderr, "probe_iframe: %zu sizes, rung %d -> %d\n", sizes.size(), before, enc.rung()); return 1; }
            std::string line = "sizes";
            for (uint32_t n : sizes) line += " " + std::to_string(n);
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
