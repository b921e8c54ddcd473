// Frame resize through include/pfv_hip.hpp (pfv::Decoder::set_output_size, pfv::frames_scale, pfv::Scaler, pfv::scale_table,
// pfv::Encoder::set_input_size): decodes a .pfv stream twice -- full-size frames, then frames resized to DW x DH -- resizes the full-size
// frames with pfv::frames_scale, and encodes the full-size frames with an encoder of DW x DH that resizes its input.
// usage: scale_report in.pfv DW DH KIND out_decoder.bin out_frames.bin out_stream.pfv     (KIND 0 bilinear, 1 bicubic, 2 Lanczos-3)
// The Python test compares the first two files with numpy's resize of the oracle decoder's frames and the third with an encoder fed those.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <sstream>

#include "pfv_hip.hpp"

static void append(std::vector<uint8_t> &to, const pfv::VideoFrame &f)
{
    to.insert(to.end(), f.plane_y.pixels.begin(), f.plane_y.pixels.end());
    to.insert(to.end(), f.plane_u.pixels.begin(), f.plane_u.pixels.end());
    to.insert(to.end(), f.plane_v.pixels.begin(), f.plane_v.pixels.end());
}

int main(int argc, char **argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: %s in.pfv DW DH KIND out_decoder.bin out_frames.bin out_stream.pfv\n", argv[0]); return 2; }
    const size_t dw = (size_t)std::atoi(argv[2]), dh = (size_t)std::atoi(argv[3]);
    const pfv::ScaleKind kind = (pfv::ScaleKind)std::atoi(argv[4]);
    try {
        pfv::Context ctx(0);
        std::ifstream in(argv[1], std::ios::binary);
        std::stringstream data;
        data << in.rdbuf();
        std::vector<uint8_t> planes, resized;
        std::vector<pfv::VideoFrame> full;
        int n = 0;
        pfv::Decoder dec(data, ctx);
        while (dec.advance_frame([&](const pfv::VideoFrame &f) { append(planes, f); full.push_back(f); })) {}
        dec.reset();
        dec.set_output_size(dw, dh, kind);
        while (dec.advance_frame([&](const pfv::VideoFrame &f) {
            if (f.width != dw || f.height != dh || f.plane_u.pixels.size() != (dw / 2) * (dh / 2)) std::exit(3);
            append(resized, f);
            n++;
        })) {}
        if (dec.width() == dw && dec.height() == dh) { std::fprintf(stderr, "width() / height() must keep the stream's size\n"); return 1; }
        // one axis' table: every row sums to 16384
        const pfv::ScaleTable t = pfv::scale_table(kind, dec.width(), dw);
        bool ok = t.taps == pfv::scale_taps(kind, dec.width(), dw) && t.first.size() == dw;
        for (size_t o = 0; o < dw && ok; o++) ok = std::accumulate(t.coef.begin() + (long)(o * t.taps), t.coef.begin() + (long)((o + 1) * t.taps), 0) == 16384;
        std::printf("frames %d of %ux%u resized to %zux%zu taps %d table %s\n", n, dec.width(), dec.height(), dw, dh, t.taps, ok ? "ok" : "BAD");
        std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<const char *>(resized.data()), (std::streamsize)resized.size());
        const std::vector<uint8_t> conv = pfv::frames_scale(ctx, dec.width(), dec.height(), dw, dh, planes, kind);
        std::ofstream(argv[6], std::ios::binary).write(reinterpret_cast<const char *>(conv.data()), (std::streamsize)conv.size());
        {
            pfv::Scaler sc(ctx, dec.width(), dec.height(), dw, dh, kind);
            if (sc.dst_frame_bytes() * (size_t)n != conv.size() || sc.src_frame_bytes() * (size_t)n != planes.size()) { std::fprintf(stderr, "Scaler: frame sizes\n"); return 1; }
        }
        std::ofstream out(argv[7], std::ios::binary);
        {
            pfv::Encoder enc(out, dw, dh, 30, 5, ctx);
            enc.set_input_size(dec.width(), dec.height(), kind);
            for (size_t k = 0; k < full.size(); k++) {
                if (k == 0) enc.encode_iframe(full[k]);
                else enc.encode_pframe(full[k]);
            }
            enc.finish();
        }
        try {
            dec.set_output_size(dw, dh, (pfv::ScaleKind)3);
            std::fprintf(stderr, "kind 3 did not throw\n");
            return 1;
        } catch (const pfv::Error &e) {
            if (e.code() != PFV_ERR_BAD_ARG) { std::fprintf(stderr, "kind 3: code %d\n", e.code()); return 1; }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
