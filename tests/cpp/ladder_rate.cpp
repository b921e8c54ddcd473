// The quality ladder through include/pfv_hip.hpp (pfv::Encoder with a ladder, set_rung, set_rate, rung): reads raw 4:2:0 frames, encodes
// frame 0 as an i-frame at START_RUNG and the rest as p-frames with the p-frame byte budget on, writes the stream to a file.
// usage: ladder_rate W H Q0,Q1,... START_RUNG PFRAME_BUDGET in.yuv out.pfv
// Prints "rungs <rung of every frame>"; the Python test compares them, and the bytes, with its own run.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: %s W H Q0,Q1,... START_RUNG PFRAME_BUDGET in.yuv out.pfv\n", argv[0]); return 2; }
    const size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    std::vector<int> qualities;
    {
        std::stringstream list(argv[3]);
        std::string item;
        while (std::getline(list, item, ',')) qualities.push_back(std::atoi(item.c_str()));
    }
    const int start_rung = std::atoi(argv[4]);
    const uint32_t budget_p = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[6], std::ios::binary);
        std::stringstream stream(std::ios::in | std::ios::out | std::ios::binary);
        pfv::Encoder enc(stream, w, h, 30, qualities, ctx);
        if (enc.n_rungs() != (int)qualities.size() || enc.rung() != 0) { std::fprintf(stderr, "ladder of %d rungs, rung %d\n", enc.n_rungs(), enc.rung()); return 1; }
        try {
            enc.set_rung(enc.n_rungs());
            std::fprintf(stderr, "set_rung past the ladder did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "set_rung past the ladder: code %d\n", e.code()); return 1; }
        }
        enc.set_rung(start_rung);
        enc.set_rate(budget_p);
        pfv::VideoFrame f(w, h);
        std::string rungs = "rungs";
        for (int t = 0;; t++) {
            in.read(reinterpret_cast<char *>(f.plane_y.pixels.data()), (std::streamsize)f.plane_y.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_u.pixels.data()), (std::streamsize)f.plane_u.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_v.pixels.data()), (std::streamsize)f.plane_v.pixels.size());
            if (!in) break;
            if (t == 0) {
                enc.encode_iframe(f);
            } else {
                enc.encode_pframe(f);
            }
            rungs += " " + std::to_string(enc.rung());
        }
        enc.finish();
        std::printf("%s\n", rungs.c_str());
        const std::string bytes = stream.str();
        std::ofstream(argv[7], std::ios::binary).write(bytes.data(), (std::streamsize)bytes.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
