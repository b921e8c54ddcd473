// Frame reports through include/pfv_hip.hpp (pfv::Encoder::set_frame_report / last_report, pfv::psnr): reads raw 4:2:0 frames, encodes
// them and prints one line per frame.  usage: quality_report W H QUALITY GOP DROP_AT DEVICE_ENTROPY in.yuv
// (frame DROP_AT becomes a drop frame; -1: none).  The Python test compares the lines with the Python Encoder's reports of the same clip.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: %s W H QUALITY GOP DROP_AT DEVICE_ENTROPY in.yuv\n", argv[0]); return 2; }
    const size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    const int quality = std::atoi(argv[3]), gop = std::atoi(argv[4]), drop_at = std::atoi(argv[5]), device_entropy = std::atoi(argv[6]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[7], std::ios::binary);
        std::stringstream stream(std::ios::in | std::ios::out | std::ios::binary);
        pfv::Encoder enc(stream, w, h, 30, quality, ctx);
        enc.set_device_entropy(device_entropy != 0);
        try {
            (void)enc.last_report();
            std::fprintf(stderr, "last_report with reports off did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_STATE) { std::fprintf(stderr, "reports off: code %d\n", e.code()); return 1; }
        }
        enc.set_frame_report(true);
        pfv::VideoFrame f(w, h);
        for (int t = 0;; t++) {
            in.read(reinterpret_cast<char *>(f.plane_y.pixels.data()), (std::streamsize)f.plane_y.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_u.pixels.data()), (std::streamsize)f.plane_u.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_v.pixels.data()), (std::streamsize)f.plane_v.pixels.size());
            if (!in) break;
            if (t == drop_at) enc.encode_dropframe();
            else if (t % gop == 0) enc.encode_iframe(f);
            else enc.encode_pframe(f);
            const pfv::FrameReport r = enc.last_report();
            const unsigned long long n = (unsigned long long)(w * h + 2 * (w / 2) * (h / 2));
            // the whole-frame figure once more through pfv::psnr: must print the same digits
            std::printf("frame %d type %d bytes %u sse %llu %llu %llu psnr %.17g %.17g %.17g yuv %.17g %.17g\n", t, r.type, r.packet_bytes,
                        (unsigned long long)r.sse[0], (unsigned long long)r.sse[1], (unsigned long long)r.sse[2], r.psnr[0], r.psnr[1], r.psnr[2],
                        r.psnr_yuv, pfv::psnr(r.sse[0] + r.sse[1] + r.sse[2], n));
        }
        enc.finish();
        std::printf("stream %zu bytes\n", stream.str().size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
