// Scene-cut detection through include/pfv_hip.hpp (pfv::Encoder::set_scene_cut / last_scene, pfv::frames_scene, pfv::scene_plan,
// pfv::SceneDetector): encodes packed frames with encode_frame under the switch, and writes the detector's own stats for the same frames.
// usage: scene_report in.yuv W H Q R THRESHOLD out.pfv out_stats.bin
// The Python test compares the stats with numpy, the plan with the restatement's, and the stream with an encoder that replays the types.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: %s in.yuv W H Q R THRESHOLD out.pfv out_stats.bin\n", argv[0]); return 2; }
    const size_t w = (size_t)std::atoi(argv[2]), h = (size_t)std::atoi(argv[3]);
    const int quality = std::atoi(argv[4]), radius = std::atoi(argv[5]);
    const uint32_t threshold = (uint32_t)std::atoi(argv[6]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const size_t fb = pfv_frame_bytes((int)w, (int)h), ny = w * h, nc = ny / 4;
        if (!fb || all.empty() || all.size() % fb) { std::fprintf(stderr, "in.yuv does not hold whole frames\n"); return 2; }
        const size_t n = all.size() / fb;
        const std::vector<pfv::SceneStats> stats = pfv::frames_scene(ctx, w, h, all, radius);
        {
            std::ofstream out(argv[7], std::ios::binary);
            pfv::Encoder enc(out, w, h, 30, quality, ctx);
            try {
                (void)enc.last_scene();
                std::fprintf(stderr, "last_scene with the switch off did not throw\n");
                return 1;
            } catch (const pfv::Error &e) {
                if (e.code() != PFV_ERR_STATE) { std::fprintf(stderr, "last_scene off: code %d\n", e.code()); return 1; }
            }
            enc.set_scene_cut(true, threshold, radius, 1);
            std::printf("types");
            for (size_t t = 0; t < n; t++) {
                pfv::VideoFrame f(w, h);
                const uint8_t *p = all.data() + t * fb;
                f.plane_y.pixels.assign(p, p + ny);
                f.plane_u.pixels.assign(p + ny, p + ny + nc);
                f.plane_v.pixels.assign(p + ny + nc, p + fb);
                std::printf(" %d", enc.encode_frame(f));
                const pfv::SceneStats got = enc.last_scene();
                if (std::memcmp(&got, &stats[t], sizeof(pfv_scene_stats)) != 0) { std::fprintf(stderr, "frame %zu: last_scene differs from frames_scene\n", t); return 1; }
            }
            std::printf("\n");
            enc.finish();
            try {
                enc.set_scene_cut(true, threshold, 8, 0);
                std::fprintf(stderr, "radius 8 did not throw\n");
                return 1;
            } catch (const pfv::Error &e) {
                if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "radius 8: code %d\n", e.code()); return 1; }
            }
        }
        std::printf("plan");
        for (uint8_t t : pfv::scene_plan(stats, threshold, 1, 0)) std::printf(" %d", (int)t);
        std::printf("\nscores");
        for (const pfv::SceneStats &s : stats) std::printf(" %u", s.score_q8());
        std::printf("\n");
        std::ofstream(argv[8], std::ios::binary).write(reinterpret_cast<const char *>(stats.data()), (std::streamsize)(stats.size() * sizeof(pfv_scene_stats)));
        pfv::SceneDetector det(ctx, w, h, 2, 4);
        det.set_radius(radius);
        det.reset(1);
        std::printf("frames %zu of %zux%zu, %zu bytes each, %zu blocks\n", n, w, h, det.frame_bytes(), det.n_blocks());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
