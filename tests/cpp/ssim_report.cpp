// Frame SSIM through include/pfv_hip.hpp (pfv::Encoder::set_frame_ssim / last_ssim, pfv::ssim, pfv::ssim_windows): reads raw 4:2:0 frames,
// encodes them and prints one line per frame.  usage: ssim_report W H QUALITY GOP DROP_AT DEVICE_ENTROPY in.yuv
// (frame DROP_AT becomes a drop frame; -1: none).  The Python test compares the lines with the Python Encoder's figures for the same clip.
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
            (void)enc.last_ssim();
            std::fprintf(stderr, "last_ssim with the switch off did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_STATE) { std::fprintf(stderr, "switch off: code %d\n", e.code()); return 1; }
        }
        enc.set_frame_ssim(true);
        const auto nw = pfv::ssim_windows(w, h);
        std::printf("windows %u %u %u\n", nw[0], nw[1], nw[2]);
        pfv::VideoFrame f(w, h);
        for (int t = 0;; t++) {
            in.read(reinterpret_cast<char *>(f.plane_y.pixels.data()), (std::streamsize)f.plane_y.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_u.pixels.data()), (std::streamsize)f.plane_u.pixels.size());
            in.read(reinterpret_cast<char *>(f.plane_v.pixels.data()), (std::streamsize)f.plane_v.pixels.size());
            if (!in) break;
            if (t == drop_at) enc.encode_dropframe();
            else if (t % gop == 0) enc.encode_iframe(f);
            else enc.encode_pframe(f);
            const pfv::FrameSsim r = enc.last_ssim();
            // the whole-frame figure once more through pfv::ssim: must print the same digits (a drop frame measures nothing and reports 1)
            const double again = t == drop_at ? 1.0 : pfv::ssim(r.q24[0] + r.q24[1] + r.q24[2], (uint64_t)nw[0] + nw[1] + nw[2]);
            std::printf("frame %d q24 %lld %lld %lld windows %u %u %u ssim %.17g %.17g %.17g all %.17g %.17g\n", t, (long long)r.q24[0],
                        (long long)r.q24[1], (long long)r.q24[2], r.windows[0], r.windows[1], r.windows[2], r.ssim[0], r.ssim[1], r.ssim[2],
                        r.ssim_all, again);
        }
        enc.finish();
        std::printf("stream %zu bytes\n", stream.str().size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
