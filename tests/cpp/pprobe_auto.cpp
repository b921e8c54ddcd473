// The p-frame size probe, the hard p-frame budget and the automatic frame type through include/pfv_hip.hpp (pfv::Encoder::probe_pframe,
// set_pframe_probe, set_gop, encode_frame): reads raw 4:2:0 frames, probes every frame as a p-frame against the encoder's reference, hands it to
// encode_frame under both byte budgets, writes the stream to a file.
// usage: pprobe_auto W H Q0,Q1,... START_RUNG IFRAME_BUDGET PFRAME_BUDGET MAX_INTERVAL in.yuv out.pfv
// Prints one line "sizes <probed bytes per rung>" per frame, then "types <type of every frame>" and "rungs <rung of every frame>"; the Python
// test compares them, and the bytes, with the model's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 10) { std::fprintf(stderr, "usage: %s W H Q0,Q1,... START_RUNG IFRAME_BUDGET PFRAME_BUDGET MAX_INTERVAL in.yuv out.pfv\n", argv[0]); return 2; }
    const size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    std::vector<int> qualities;
    {
        std::stringstream list(argv[3]);
        std::string item;
        while (std::getline(list, item, ',')) qualities.push_back(std::atoi(item.c_str()));
    }
    const int start_rung = std::atoi(argv[4]);
    const uint32_t budget_i = (uint32_t)std::strtoul(argv[5], nullptr, 10), budget_p = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    const int max_interval = std::atoi(argv[7]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[8], std::ios::binary);
        std::stringstream stream(std::ios::in | std::ios::out | std::ios::binary);
        pfv::Encoder enc(stream, w, h, 30, qualities, ctx);
        enc.set_rung(start_rung);
        enc.set_iframe_budget(budget_i);
        enc.set_rate(budget_p);
        enc.set_pframe_probe(true);
        enc.set_gop(max_interval);
        pfv::VideoFrame f(w, h);
        std::string types = "types", rungs = "rungs";
        for (;;) {
            in.read(reinterpret_cast<char *>(f.plane_y.pixels.data()), (std::streamsize)f.plane_y.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_u.pixels.data()), (std::streamsize)f.plane_u.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_v.pixels.data()), (std::streamsize)f.plane_v.pixels.size());
            if (!in) break;
            const int before = enc.rung();
            const std::vector<uint32_t> sizes = enc.probe_pframe(f);
            if (sizes.size() != qualities.size() || enc.rung() != before) { std::fprintf(stderr, "probe_pframe: %zu sizes, rung %d -> %d\n", sizes.size(), before, enc.rung()); return 1; }
            std::string line = "sizes";
            for (uint32_t n : sizes) line += " " + std::to_string(n);
            std::printf("%s\n", line.c_str());
            types += " " + std::to_string(enc.encode_frame(f));
            rungs += " " + std::to_string(enc.rung());
        }
        enc.finish();
        std::printf("%s\n%s\n", types.c_str(), rungs.c_str());
        const std::string bytes = stream.str();
        std::ofstream(argv[9], std::ios::binary).write(bytes.data(), (std::streamsize)bytes.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
