// RGB / RGBA texture output through include/pfv_hip.hpp (pfv::Decoder::set_output_rgb, pfv::frames_to_rgb, pfv::rgb_row_bytes): decodes a .pfv
// stream twice -- planes, then pictures in the given format -- and converts the planes with pfv::frames_to_rgb.
// usage: present_report in.pfv FORMAT out_pictures.bin out_converted.bin     (FORMAT 0 RGB8, 1 RGBA8, 2 BGRA8)
// The Python test compares both files with the numpy oracle's conversion of the oracle decoder's frames.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s in.pfv FORMAT out_pictures.bin out_converted.bin\n", argv[0]); return 2; }
    const pfv::PixelFormat fmt = (pfv::PixelFormat)std::atoi(argv[2]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[1], std::ios::binary);
        std::stringstream data;
        data << in.rdbuf();
        std::vector<uint8_t> planes, pictures;
        int n = 0, n_rgb = 0;
        {
            pfv::Decoder dec(data, ctx);
            while (dec.advance_frame([&](const pfv::VideoFrame &f) {
                planes.insert(planes.end(), f.plane_y.pixels.begin(), f.plane_y.pixels.end());
                planes.insert(planes.end(), f.plane_u.pixels.begin(), f.plane_u.pixels.end());
                planes.insert(planes.end(), f.plane_v.pixels.begin(), f.plane_v.pixels.end());
                n++;
            })) {}
        }
        data.clear();
        data.seekg(0);
        pfv::Decoder dec(data, ctx);
        dec.set_output_rgb(true, fmt);
        try {
            dec.advance_frame([](const pfv::VideoFrame &) {});
            std::fprintf(stderr, "advance_frame with the RGB switch on did not throw\n");
            return 1;
        } catch (const std::logic_error &) {
        }
        while (dec.advance_frame_rgb([&](const std::vector<uint8_t> &px, uint32_t w, uint32_t h) {
            if (px.size() != pfv::rgb_row_bytes(w, fmt) * h) std::exit(3);
            pictures.insert(pictures.end(), px.begin(), px.end());
            n_rgb++;
        })) {}
        std::printf("frames %d pictures %d of %ux%u row %zu\n", n, n_rgb, dec.width(), dec.height(), pfv::rgb_row_bytes(dec.width(), fmt));
        std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char *>(pictures.data()), (std::streamsize)pictures.size());
        const std::vector<uint8_t> conv = pfv::frames_to_rgb(ctx, dec.width(), dec.height(), planes, fmt);
        std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(conv.data()), (std::streamsize)conv.size());
        try {
            dec.set_output_rgb(true, (pfv::PixelFormat)3);
            std::fprintf(stderr, "format 3 did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "format 3: code %d\n", e.code()); return 1; }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
