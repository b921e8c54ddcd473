// The hierarchical motion search through include/pfv_hip.hpp (pfv::EncoderSession / pfv::Encoder / pfv::GopEncoder ::set_motion_search,
// pfv::EncoderSession::coarse_vectors): packed frames (frame 0 an i-frame, the rest p-frames) in HIER mode at radius R; prints every p-frame's
// vectors, coarse vectors and coded count from the session and every packet's size from the stream encoder, and checks that pfv::GopEncoder
// writes the same stream.
// usage: hier_report in.yuv W H Q R
// The Python test compares the output line by line with the Python path's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>

#include "pfv_hip.hpp"

int main(int argc, char **argv)
{
    if (argc != 6) { std::fprintf(stderr, "usage: %s in.yuv W H Q R\n", argv[0]); return 2; }
    const size_t w = (size_t)std::atoi(argv[2]), h = (size_t)std::atoi(argv[3]);
    const int quality = std::atoi(argv[4]), radius = std::atoi(argv[5]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const size_t fb = pfv_frame_bytes((int)w, (int)h), ny = w * h, nc = ny / 4;
        if (!fb || all.empty() || all.size() % fb) { std::fprintf(stderr, "in.yuv does not hold whole frames\n"); return 2; }
        const size_t n = all.size() / fb;
        auto frame = [&](size_t t) {
            pfv::VideoFrame f(w, h);
            const uint8_t *p = all.data() + t * fb;
            f.plane_y.pixels.assign(p, p + ny);
            f.plane_u.pixels.assign(p + ny, p + ny + nc);
            f.plane_v.pixels.assign(p + ny + nc, p + fb);
            return f;
        };
        pfv::EncoderSession sess(ctx, w, h, quality);
        std::ostringstream out, gout;
        pfv::Encoder enc(out, w, h, 30, quality, ctx);
        sess.set_motion_search(pfv::MotionSearch::Hier, radius);
        enc.set_motion_search(pfv::MotionSearch::Hier, radius);
        for (size_t t = 0; t < n; t++) {
            const std::vector<uint8_t> packed(all.begin() + (long)(t * fb), all.begin() + (long)((t + 1) * fb));
            const size_t before = out.str().size();
            if (t == 0) {
                sess.encode_iframe(packed);
                enc.encode_iframe(frame(t));
            } else {
                const pfv::EncoderSession::PFrame p = sess.encode_pframe(packed);
                enc.encode_pframe(frame(t));
                std::printf("frame %zu mv", t);
                size_t coded = 0;
                for (size_t i = 0; i < sess.total_blocks(); i++) {
                    std::printf(" %d,%d", (int)p.mv[2 * i], (int)p.mv[2 * i + 1]);
                    coded += p.has_coef[i];
                }
                const std::vector<int8_t> cv = sess.coarse_vectors();
                std::printf("\nframe %zu coarse", t);
                for (size_t i = 0; i < sess.total_blocks(); i++) std::printf(" %d,%d", (int)cv[2 * i], (int)cv[2 * i + 1]);
                std::printf("\nframe %zu coded %zu\n", t, coded);
            }
            std::printf("frame %zu packet %zu\n", t, out.str().size() - before);
        }
        enc.finish();
        {
            pfv::GopEncoder gop(gout, w, h, 30, quality, ctx, 2, 2);
            gop.set_motion_search(pfv::MotionSearch::Hier, radius);
            for (size_t t = 0; t < n; t++) {
                if (t == 0) gop.encode_iframe(frame(t)); else gop.encode_pframe(frame(t));
            }
            gop.finish();
        }
        if (gout.str() != out.str()) { std::fprintf(stderr, "pfv::GopEncoder wrote another stream\n"); return 1; }
        std::printf("gop stream %zu bytes identical\n", out.str().size());
        const auto mode = sess.motion_search();
        std::printf("mode %s radius %d\n", mode.first == pfv::MotionSearch::Hier ? "hier" : "other", mode.second);
        try {
            sess.set_motion_search(pfv::MotionSearch::Hier, 7);
            std::fprintf(stderr, "radius 7 did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "radius 7: code %d\n", e.code()); return 1; }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
