// Out-of-loop deblocking through include/pfv_hip.hpp (pfv::Decoder::set_deblock, pfv::frames_deblock, pfv::deblock_strength): decodes a .pfv
// stream with the switch in the given mode and writes every frame the callback receives, then the filter alone on those frames.
// usage: deblock_report in.pfv MODE SY SU SV Q0 out.yuv out_filtered.yuv     (MODE 0 off, 1 auto, 2 fixed; Q0: a DC quantiser)
// The Python test compares the files with the Python Decoder's frames and with numpy.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: %s in.pfv MODE SY SU SV Q0 out.yuv out_filtered.yuv\n", argv[0]); return 2; }
    const int mode = std::atoi(argv[2]);
    const std::array<uint8_t, 3> st = {(uint8_t)std::atoi(argv[3]), (uint8_t)std::atoi(argv[4]), (uint8_t)std::atoi(argv[5])};
    try {
        pfv::Context ctx(0);
        int32_t table[64];
        for (int i = 0; i < 64; i++) table[i] = 99;
        table[0] = std::atoi(argv[6]);
        std::printf("strength %d\n", pfv::deblock_strength(table));
        std::ifstream in(argv[1], std::ios::binary);
        pfv::Decoder dec(in, ctx);
        dec.set_deblock((pfv::Deblock)mode, st);
        std::vector<uint8_t> all;
        int n = 0;
        auto take = [&](const pfv::VideoFrame &f) {
            all.insert(all.end(), f.plane_y.pixels.begin(), f.plane_y.pixels.end());
            all.insert(all.end(), f.plane_u.pixels.begin(), f.plane_u.pixels.end());
            all.insert(all.end(), f.plane_v.pixels.begin(), f.plane_v.pixels.end());
            n++;
        };
        while (dec.advance_frame(take)) {}
        std::printf("frames %d of %ux%u\n", n, dec.width(), dec.height());
        std::ofstream(argv[7], std::ios::binary).write(reinterpret_cast<const char *>(all.data()), (std::streamsize)all.size());
        const std::vector<uint8_t> filtered = pfv::frames_deblock(ctx, dec.width(), dec.height(), all, st);
        std::ofstream(argv[8], std::ios::binary).write(reinterpret_cast<const char *>(filtered.data()), (std::streamsize)filtered.size());
        try {
            dec.set_deblock(pfv::Deblock::Fixed, {0, 13, 0});
            std::fprintf(stderr, "strength 13 did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "strength 13: code %d\n", e.code()); return 1; }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
