// RGB / RGBA picture input through include/pfv_hip.hpp (pfv::frames_from_rgb, pfv::Encoder::set_input_rgb): converts tight pictures to packed
// frames and encodes them -- the first as an i-frame, the others as p-frames -- into a .pfv stream.
// usage: ingest_report WIDTH HEIGHT FORMAT CHROMA QUALITY in_pictures.bin out_frames.bin out.pfv
//        (FORMAT 0 RGB8, 1 RGBA8, 2 BGRA8; CHROMA 0 point, 1 box)
// The Python test compares both files with what the Python mirror made of the same pictures.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: %s WIDTH HEIGHT FORMAT CHROMA QUALITY in_pictures.bin out_frames.bin out.pfv\n", argv[0]); return 2; }
    const size_t w = (size_t)std::atoi(argv[1]), h = (size_t)std::atoi(argv[2]);
    const pfv::PixelFormat fmt = (pfv::PixelFormat)std::atoi(argv[3]);
    const pfv::ChromaMode chroma = (pfv::ChromaMode)std::atoi(argv[4]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[6], std::ios::binary);
        const std::vector<uint8_t> pictures((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const size_t pic = pfv::rgb_row_bytes(w, fmt) * h;
        if (!pic || pictures.empty() || pictures.size() % pic) { std::fprintf(stderr, "the input does not hold whole pictures\n"); return 2; }
        const std::vector<uint8_t> frames = pfv::frames_from_rgb(ctx, w, h, pictures, fmt, chroma);
        std::ofstream(argv[7], std::ios::binary).write(reinterpret_cast<const char *>(frames.data()), (std::streamsize)frames.size());
        std::ofstream out(argv[8], std::ios::binary);
        pfv::Encoder enc(out, w, h, 30, std::atoi(argv[5]), ctx);
        try {
            enc.encode_iframe_rgb(std::vector<uint8_t>(pictures.begin(), pictures.begin() + (std::ptrdiff_t)pic));
            std::fprintf(stderr, "encode_iframe_rgb with the switch off did not throw\n");
            return 1;
        } catch (const std::logic_error &) {
        }
        try {
            enc.set_input_rgb(true, fmt, (pfv::ChromaMode)2);
            std::fprintf(stderr, "chroma mode 2 did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "chroma mode 2: code %d\n", e.code()); return 1; }
        }
        enc.set_input_rgb(true, fmt, chroma);
        size_t n = 0;
        for (size_t at = 0; at < pictures.size(); at += pic, n++) {
            const std::vector<uint8_t> one(pictures.begin() + (std::ptrdiff_t)at, pictures.begin() + (std::ptrdiff_t)(at + pic));
            if (n == 0) enc.encode_iframe_rgb(one);
            else enc.encode_pframe_rgb(one);
        }
        enc.finish();
        std::printf("pictures %zu of %zux%zu picture bytes %zu frame bytes %zu\n", n, w, h, pic, frames.size() / n);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
