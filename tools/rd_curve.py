#!/usr/bin/env python3
"""Rate / distortion of the codec over its quality setting, measured on the device.

    python tools/rd_curve.py WIDTH HEIGHT FRAMES [--gop G] [--kind pan|low_motion|static] [--qualities 0,2,5,10] [--time-kernel]

Per quality the synthetic clip goes through ``Encoder`` with frame reports on (pfv_encoder_set_frame_report: the k_sse_* kernels
compare every frame with the reconstruction the encoder leaves behind); one JSON line per quality: bytes per frame, split into
i-frames and p-frames, and the mean PSNR of Y, U, V and of the whole frame.

--time-kernel (on the GPU box) adds one more line: the k_sse_mb + k_sse_sum pair at the benched shape -- 96 streams of 1920 x 1080,
input packed, reconstruction padded, map to scratch -- against pfv_dec_get_frame_dev (k_crop_frames) over the same 96 frames, which
moves the same bytes; HIP events around every launch, warm-up, median of the samples.  And what the reports cost pfv_encoder per
frame at 1080p (host clock around calls that end in a synchronise), against the same encoder with reports off.
"""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g   # noqa: E402


def load():
    pkg = g.load_package()
    if not __import__("libswitch").apply_from_env(pkg):      # PFV_HIP_LIB=<another build of the C ABI> (tests: the CPU emulator)
        g.build_hip()
    return pkg


def encode_clip(pkg, ctx, w, h, n_frames, gop, kind, quality, frame_report=True):
    """-> (stream bytes, reports, seconds per encode call)"""
    st = pkg.SyntheticStream(w, h, kind=kind)
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, frame_report=frame_report)
    reports, secs = [], []
    for t in range(n_frames):
        fr = pkg.VideoFrame.from_packed(w, h, st.frame(t))
        t0 = time.perf_counter()
        (enc.encode_iframe if t % gop == 0 else enc.encode_pframe)(fr)
        secs.append(time.perf_counter() - t0)
        if frame_report:
            reports.append(enc.last_report)
    enc.finish()
    enc.close()
    return buf.getvalue(), reports, secs


def rd_line(pkg, ctx, w, h, n_frames, gop, kind, quality):
    data, reports, _ = encode_clip(pkg, ctx, w, h, n_frames, gop, kind, quality)
    by = {1: [r.packet_bytes for r in reports if r.type == 1], 2: [r.packet_bytes for r in reports if r.type == 2]}
    mean = lambda v: float(sum(v) / len(v)) if v else None   # noqa: E731
    return {"quality": quality, "width": w, "height": h, "frames": n_frames, "gop": gop, "kind": kind,
            "stream_bytes": len(data), "packet_bytes": sum(r.packet_bytes for r in reports),
            "bytes_per_frame": mean([r.packet_bytes for r in reports]),
            "iframes": len(by[1]), "iframe_bytes_per_frame": mean(by[1]), "pframes": len(by[2]), "pframe_bytes_per_frame": mean(by[2]),
            "psnr_y": mean([r.psnr[0] for r in reports]), "psnr_u": mean([r.psnr[1] for r in reports]),
            "psnr_v": mean([r.psnr[2] for r in reports]), "psnr_yuv": mean([r.psnr_yuv for r in reports])}


def time_kernels(pkg, ctx, n_streams=96, w=1920, h=1080, warmup=5, samples=30):
    lib = ctx._lib
    fb = int(lib.pfv_frame_bytes(w, h))
    tb = int(lib.pfv_total_blocks(w, h))
    frames = ctx.alloc(fb * n_streams)
    coef = ctx.alloc(n_streams * tb * 512)
    sse = ctx.alloc(n_streams * 24)
    out = ctx.alloc(fb * n_streams)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, frames)
    enc = pkg.EncoderSession(ctx, w, h, 5, n_streams)
    dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(5)[:4]), n_streams)
    enc.encode_iframe_dev(frames, coef)           # prev_frame = the reconstruction of `frames`
    dec.decode_iframe_dev(coef)                   # framebuffer = the same frames, decoded
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()

    def median_ms(fn):
        got = []
        for k in range(warmup + samples):
            ctx.record(e0)
            fn()
            ctx.record(e1)
            ms = ctypes.c_float()
            ctx.check(lib.pfv_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            if k >= warmup:
                got.append(float(ms.value))
        return statistics.median(got), min(got), max(got)
    # alternate the two, so that whatever else the box is doing meets both
    res = {"sse": [], "crop": []}
    for _ in range(3):
        res["sse"].append(median_ms(lambda: enc.distortion_dev(frames, sse)))
        res["crop"].append(median_ms(lambda: dec.get_frame_dev(out)))
    sums = np.zeros((n_streams, 3), dtype=np.uint64)
    ctx.download(sums, sse)
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    enc.close(); dec.close()
    for p in (frames, coef, sse, out):
        ctx.free(p)
    sse_ms = statistics.median(m for m, _, _ in res["sse"])
    crop_ms = statistics.median(m for m, _, _ in res["crop"])
    bytes_moved = n_streams * (fb + int(lib.pfv_padded_frame_bytes(w, h)))
    line = {"shape": f"{n_streams} x {w}x{h}", "samples_per_round": samples, "rounds": 3,
            "sse_pair_ms": sse_ms, "crop_ms": crop_ms, "ratio": sse_ms / crop_ms,
            "sse_rounds_ms": res["sse"], "crop_rounds_ms": res["crop"], "bytes_per_launch": bytes_moved,
            "sse_GBps": bytes_moved / sse_ms / 1e6, "crop_GBps": bytes_moved / crop_ms / 1e6,
            "psnr_y_stream0": pkg.psnr(int(sums[0, 0]), w * h)}
    # what the reports cost pfv_encoder: per encode call at 1080p, GOP 15, reports off / on alternating
    per = {False: [], True: []}
    for _ in range(3):
        for on in (False, True):
            _, _, secs = encode_clip(pkg, ctx, w, h, 30, 15, "pan", 5, frame_report=on)
            per[on].append(statistics.median(secs[2:]) * 1e3)
    line["encoder_ms_per_frame_reports_off"] = statistics.median(per[False])
    line["encoder_ms_per_frame_reports_on"] = statistics.median(per[True])
    line["encoder_rounds_ms"] = {"off": per[False], "on": per[True]}
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("frames", type=int)
    ap.add_argument("--gop", type=int, default=15)
    ap.add_argument("--kind", choices=("pan", "low_motion", "static"), default="pan")
    ap.add_argument("--qualities", default="0,2,5,10")
    ap.add_argument("--time-kernel", action="store_true")
    a = ap.parse_args()
    assert a.frames >= 1 and a.gop >= 1
    pkg = load()
    with pkg.Context(0) as ctx:
        for q in [int(x) for x in a.qualities.split(",") if x != ""]:
            print(json.dumps(rd_line(pkg, ctx, a.width, a.height, a.frames, a.gop, a.kind, q)), flush=True)
        if a.time_kernel:
            print(json.dumps({"time_kernel": time_kernels(pkg, ctx)}), flush=True)


if __name__ == "__main__":
    main()
