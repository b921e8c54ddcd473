// A poisoned pfv_encoder (tests/cpp/poison_seam.h fails the payload-size download of a p-frame behind its encode kernel): the p-frame probe and
// encode_pframe return PFV_ERR_STATE, nothing was written, and pfv_encoder_encode_frame recovers with an i-frame -- on the entropy path named
// by DEVICE_ENTROPY -- after which the probe and the automatic frame type work again.
// usage: pprobe_poison W H Q0,Q1,... DEVICE_ENTROPY in.yuv out.pfv      (three frames; linked against the seam build of the emulator library)
// Prints "failed <rc>", "poisoned <rc of probe_pframe> <rc of encode_pframe> <bytes written by the failed call>", "type <of frame 1>",
// "sizes <probe of frame 2>", "type <of frame 2>"; the Python test compares them, and the stream bytes, with the model's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "pfv_hip.h"

extern int pfv_seam_fail_d2h;

#define CHECK(expr)                                                                                         \
    do {                                                                                                    \
        int rc__ = (expr);                                                                                  \
        if (rc__ != PFV_OK) { std::fprintf(stderr, "%s -> %d\n", #expr, rc__); return 1; }                  \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: %s W H Q0,Q1,... DEVICE_ENTROPY in.yuv out.pfv\n", argv[0]); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
    std::vector<int> q;
    {
        std::stringstream list(argv[3]);
        std::string item;
        while (std::getline(list, item, ',')) q.push_back(std::atoi(item.c_str()));
    }
    const int recover_on_device = std::atoi(argv[4]);
    const size_t ny = (size_t)w * h, nc = (size_t)(w / 2) * (h / 2), fb = ny + 2 * nc;
    std::vector<uint8_t> clip(3 * fb);
    if (!std::ifstream(argv[5], std::ios::binary).read(reinterpret_cast<char *>(clip.data()), (std::streamsize)clip.size())) return 2;
    auto Y = [&](int t) { return clip.data() + t * fb; };
    auto U = [&](int t) { return clip.data() + t * fb + ny; };
    auto V = [&](int t) { return clip.data() + t * fb + ny + nc; };

    pfv_ctx *ctx = nullptr;
    pfv_encoder *e = nullptr;
    CHECK(pfv_ctx_create(0, &ctx));
    CHECK(pfv_encoder_create_ladder(ctx, w, h, 30, q.data(), (int)q.size(), &e));
    CHECK(pfv_encoder_set_rung(e, 1));
    CHECK(pfv_encoder_encode_iframe(e, Y(0), U(0), V(0)));
    const uint8_t *data = nullptr;
    size_t before = 0, after = 0;
    CHECK(pfv_encoder_bytes(e, &data, &before));

    pfv_seam_fail_d2h = 1;                                        // the payload size of the next frame does not come down
    const int failed = pfv_encoder_encode_pframe(e, Y(1), U(1), V(1));
    if (pfv_seam_fail_d2h != 0) { std::fprintf(stderr, "the seam was not reached\n"); return 1; }
    std::printf("failed %d\n", failed);
    std::vector<uint32_t> sizes(q.size());
    const int rc_probe = pfv_encoder_probe_pframe(e, Y(1), U(1), V(1), sizes.data());
    const int rc_p = pfv_encoder_encode_pframe(e, Y(1), U(1), V(1));
    CHECK(pfv_encoder_bytes(e, &data, &after));
    std::printf("poisoned %d %d %zu\n", rc_probe, rc_p, after - before);

    CHECK(pfv_encoder_set_device_entropy(e, recover_on_device));
    int type = 0;
    CHECK(pfv_encoder_encode_frame(e, Y(1), U(1), V(1), &type));
    std::printf("type %d\n", type);
    CHECK(pfv_encoder_probe_pframe(e, Y(2), U(2), V(2), sizes.data()));
    std::string line = "sizes";
    for (uint32_t n : sizes) line += " " + std::to_string(n);
    std::printf("%s\n", line.c_str());
    CHECK(pfv_encoder_encode_frame(e, Y(2), U(2), V(2), &type));
    std::printf("type %d\n", type);
    CHECK(pfv_encoder_finish(e));
    CHECK(pfv_encoder_bytes(e, &data, &after));
    std::ofstream(argv[6], std::ios::binary).write(reinterpret_cast<const char *>(data), (std::streamsize)after);
    pfv_encoder_destroy(e);
    pfv_ctx_destroy(ctx);
    return 0;
}
