// The denoising pre-filter through include/pfv_hip.hpp (pfv::Encoder::set_denoise, pfv::frames_denoise, pfv::Denoiser): encodes packed frames
// with the switch on, and writes the filter's own output for the same frames.
// usage: denoise_report in.yuv W H Q SY SU SV TY TU TV out.pfv out_filtered.yuv     (frame 0 and every third frame are i-frames)
// The Python test compares the stream with a plain encoder fed numpy's frames, and the frames with numpy.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 13) { std::fprintf(stderr, "usage: %s in.yuv W H Q SY SU SV TY TU TV out.pfv out_filtered.yuv\n", argv[0]); return 2; }
    const size_t w = (size_t)std::atoi(argv[2]), h = (size_t)std::atoi(argv[3]);
    const int quality = std::atoi(argv[4]);
    const std::array<uint8_t, 3> sp = {(uint8_t)std::atoi(argv[5]), (uint8_t)std::atoi(argv[6]), (uint8_t)std::atoi(argv[7])};
    const std::array<uint8_t, 3> tp = {(uint8_t)std::atoi(argv[8]), (uint8_t)std::atoi(argv[9]), (uint8_t)std::atoi(argv[10])};
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const size_t fb = pfv_frame_bytes((int)w, (int)h), ny = w * h, nc = ny / 4;
        if (!fb || all.empty() || all.size() % fb) { std::fprintf(stderr, "in.yuv does not hold whole frames\n"); return 2; }
        const size_t n = all.size() / fb;
        {
            std::ofstream out(argv[11], std::ios::binary);
            pfv::Encoder enc(out, w, h, 30, quality, ctx);
            enc.set_denoise(true, sp, tp);
            for (size_t t = 0; t < n; t++) {
                pfv::VideoFrame f(w, h);
                const uint8_t *p = all.data() + t * fb;
                f.plane_y.pixels.assign(p, p + ny);
                f.plane_u.pixels.assign(p + ny, p + ny + nc);
                f.plane_v.pixels.assign(p + ny + nc, p + fb);
                if (t % 3 == 0) enc.encode_iframe(f); else enc.encode_pframe(f);
            }
            enc.finish();
            try {
                enc.set_denoise(true, {0, 17, 0}, tp);
                std::fprintf(stderr, "strength 17 did not throw\n");
                return 1;
            } catch (const pfv::Error &e) {
                if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "strength 17: code %d\n", e.code()); return 1; }
            }
        }
        const std::vector<uint8_t> filtered = pfv::frames_denoise(ctx, w, h, all, sp, tp);
        std::ofstream(argv[12], std::ios::binary).write(reinterpret_cast<const char *>(filtered.data()), (std::streamsize)filtered.size());
        pfv::Denoiser dn(ctx, w, h, 2);
        dn.set_strength(sp, tp);
        dn.reset(1);
        std::printf("frames %zu of %zux%zu, %zu bytes each\n", n, w, h, dn.frame_bytes());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
