#!/usr/bin/env python3
"""Rate / distortion of the codec over its quality setting, measured on the device.

    python tools/rd_curve.py WIDTH HEIGHT FRAMES [--gop G] [--kind pan|low_motion|static] [--qualities 0,2,5,10] [--time-kernel] [--probe] [--probe-p] [--probe-rd] [--probe-p-rd] [--ssim] [--time-ssim] [--deblock] [--dump DIR] [--time-deblock] [--time-present] [--time-ingest] [--time-scale] [--denoise SS,ST] [--time-denoise] [--search full[,R]|hier,R] [--pan DX,DY] [--time-search] [--scene-cut [THRESHOLD,R]] [--time-scene]

Per quality the synthetic clip goes through ``Encoder`` with frame reports on (pfv_encoder_set_frame_report: the k_sse_* kernels
compare every frame with the reconstruction the encoder leaves behind); one JSON line per quality: bytes per frame, split into
i-frames and p-frames, and the mean PSNR of Y, U, V and of the whole frame.

--ssim adds ssim_y, ssim_u, ssim_v and ssim_all to each line: the mean over the frames of the per-frame structural similarity
(pfv_encoder_set_frame_ssim: the k_ssim_* kernels on the same pair of frames).  Without the flag the lines are what they were.

--time-ssim (on the GPU box) adds one more line: the k_ssim_mb + k_ssim_sum pair against the k_sse_mb + k_sse_sum pair on the same buffers
at the benched shape (96 x 1080p, input packed, reconstruction padded, maps to scratch), HIP events around every launch pair, warm-up, the
MEAN of the samples, the two alternating in three rounds; both times, their ratio and the bytes per second each implies.

--deblock adds, per quality, the PSNR and SSIM of the DEBLOCKED reconstruction (db_psnr_*, db_ssim_*) next to the plain ones (psnr_*, ssim_*),
and the strengths used (db_strength_i / _p): an encoder session's prev_frame as PADDED source -> pfv_frames_deblock_dev at the automatic
strengths (pfv_deblock_strength) of the frame's tables -> pfv_frames_sse_dev / pfv_frames_ssim_dev against the input.  --dump DIR writes
what was measured as raw packed frames: q<quality>_input.yuv, q<quality>_recon.yuv (prev_frame cropped), q<quality>_deblocked.yuv.

--time-deblock (on the GPU box) adds one more line: k_deblock against k_crop_frames on the same 96 x 1080p launch -- pfv_dec_get_frame_dev of
one decoder session with the switch fixed at (5, 10, 10), at (0, 0, 0) (the copy path) and off -- HIP events around every launch, warm-up, the
median of the samples, alternating in three rounds; and pfv_dec_pframe_dev with an output buffer set, switch off (fused crop) against auto.

--denoise SS,ST adds, per quality, what the denoising pre-filter (pfv_encoder_set_denoise, spatial strength SS and temporal ST on every plane)
does to the clip PLUS seeded uniform noise in [-3, 3]: stream bytes and bytes per frame of the noisy clip without (noisy_*) and with the filter
(dn_*), the PSNR of the encoder's input against the CLEAN clip (noisy_psnr_clean, dn_psnr_clean) and the share of p-frame macroblocks that are
skipped (noisy_skipped_share, dn_skipped_share).  --dump DIR also writes q<quality>_clean.yuv, _noisy.yuv and _denoised.yuv.

--time-denoise (on the GPU box) adds one more line: k_denoise (committed, steady state, strengths 6 / 6, packed and padded source) beside
k_deblock and k_crop_frames on the same 96 x 1080p frames -- HIP events on the context's stream around every launch, warm-up, the median of
the samples, alternating in three rounds.  With PFV_HIP_LIB set only one WIDTH x HEIGHT stream runs: the row is printed, its times mean nothing.

--scene-cut [THRESHOLD,R] (default 176,5) adds, per quality, one line {"scene_cut": ...}: a clip spliced in segments from
SyntheticStream(SEED, "pan") and SyntheticStream(SEED + 17, "low_motion") (WIDTH x HEIGHT, FRAMES frames; "splices" names the frames) is measured by
pfv_frames_scene at radius R ("scores_q8") and encoded twice through pfv_encoder with explicit types: an i-frame every 15 frames (fixed_*) and the
types pfv_scene_plan makes of the stats at THRESHOLD, min_interval 1, max_interval 15 (planned_*): bytes, i-frames, worst and mean PSNR-YUV of the
frame reports.

--time-scene (on the GPU box) adds one more line: the three scene kernels on 96 x 1080p frames in HBM (pfv_scene_detector_run_dev, uncommitted,
steady state, R = 4 and R = 7) and on one 4K x 60-frame clip (pfv_scene_detector_run_clip_dev, R = 4) -- per kernel from the events
pfv_scene_detector_run_timed_dev records between them, per launch group from an event pair -- beside the k_sse_mb + k_sse_sum pair on the same two
frames and the default p-frame encode; warm-up, the median of the samples, alternating in three rounds.  With PFV_HIP_LIB set two WIDTH x HEIGHT
streams and a three-frame clip run: the row is printed, its times mean nothing.

--search full[,R] (R = 1 .. 15, default 15) adds, per quality, the clip encoded with both motion searches (pfv_encoder_set_motion_search) side by
side: four_ / full_ stream_bytes, psnr_yuv (mean over the frames, frame reports), and the coded and skipped p-frame macroblocks (an encoder
session fed the same frames); search_radius = R.

--search hier,R (R even, 2 .. 62) adds the same columns for three encoders: four_ (four-step), full_ (PFV_SEARCH_FULL at radius 15) and hier_
(PFV_SEARCH_HIER at radius R).  --pan DX,DY replaces the clip of the --search columns by a textured canvas seen through a window that moves by
(DX, DY) pixels per frame (search_pan = [DX, DY]): a pan beyond +-15 is what the two-level search is for.

--time-search also times PFV_SEARCH_HIER at radius 30 and 62: the whole p-frame launch (hier_r30_ms, hier_r62_ms) and, from
pfv_enc_pframe_hier_timed_dev, its five kernels (hier_r30_stages_ms / hier_r62_stages_ms: k_halve of the source, k_halve of the reference,
k_pf_search_coarse, k_pf_refine, k_pf_transform), with the v_dot4 floor of the coarse level's products ((2 Rc + 1)^2 x 16 per macroblock).

--time-search (on the GPU box) adds one more line: k_pf_search_full + k_pf_transform at R = 7 and R = 15 against the default p-frame encode of
the same 96 x 1080p frames (frame 1 of the synthetic streams behind frame 0 as an i-frame) -- HIP events on the context's stream around every
pfv_enc_pframe_dev, warm-up, the median of the samples, the three alternating in three rounds; the ratios to the default encode and to the
v_dot4 issue floor of the products alone ((2R + 1)^2 x 64 per macroblock over its 8 lanes, 4.2 cycles each, 1 024 SIMDs, 2.4 GHz).  With PFV_HIP_LIB set only two
WIDTH x HEIGHT streams run: the row is printed, its times mean nothing.

--time-present (on the GPU box) adds six lines, one per pixel format (RGB8, RGBA8, BGRA8) on 96 x 1080p and on one WIDTH x HEIGHT stream: the
RGB pictures of a decoder session's frames (a) by pfv_dec_get_frame_rgb_dev -- one k_present_rgb from the padded framebuffer; (b) the way without
it -- pfv_dec_get_frame_dev (k_crop_frames) plus one pfv_yuv420_to_rgb_dev per stream, which gives RGB8 only; (c) pfv_dec_get_frame_dev alone.
HIP events around each, warm-up, the median of the samples, a / b / c alternating in three rounds; milliseconds, the bytes each must move
(picture bytes read + bytes written) over its time, and (a)'s rate as a fraction of (c)'s.  With PFV_HIP_LIB set (another build of the C ABI:
the CPU emulator) only the small shape runs, twice: the rows are printed, their times mean nothing.

--time-ingest (on the GPU box) adds twelve lines, one per pixel format and chroma mode (point, box) on 96 x 1080p and on one WIDTH x HEIGHT
stream: planar frames from RGB pictures (a) by pfv_frames_from_rgb_dev -- one k_ingest_rgb; (b) the way without it -- one pfv_rgb_to_yuv420_dev
per stream, which takes RGB8 and gives POINT only (the same figure beside every format and mode); (c) pfv_frames_to_rgb_dev on the same shape
and format: the same bytes in the other direction.  Method, units and the PFV_HIP_LIB rule as --time-present; (a)'s rate as a fraction of (c)'s.

--time-kernel (on the GPU box) adds one more line: the k_sse_mb + k_sse_sum pair at the benched shape -- 96 streams of 1920 x 1080,
input packed, reconstruction padded, map to scratch -- against pfv_dec_get_frame_dev (k_crop_frames) over the same 96 frames, which
moves the same bytes; HIP events around every launch, warm-up, median of the samples.  And what the reports cost pfv_encoder per
frame at 1080p (host clock around calls that end in a synchronise), against the same encoder with reports off.

--probe: the i-frame size probe (pfv_encoder_probe_iframe) on the clip's first frame with --qualities as the ladder -- probed against written
payload bytes per rung (frame reports) -- and then its timing (on the GPU box): A = the probe's two launches (k_probe_iframe + k_probe_sizes)
against B = what the tree offered before for the same answer, per rung pfv_enc_iframe_dev + the entropy stage, at 96 x 1080p and 1 x 1080p,
ladders 0,2,5,7,10 and 0..10.  B twice: with the stage as a caller runs it (all four k_ent_* kernels), and with a payload capacity of 24 bytes,
where k_ent_init / k_ent_pack leave at once -- the stage "up to the size" (k_ent_scan + k_ent_codes), B's lower bound.  HIP events on the
context's stream, warm-up, A and B alternating in one process, medians; the whole comparison three times for B's own spread.  Last the
latency an i-frame budget adds to one pfv_encoder at 1080p (host clock, budget off / on alternating).

--probe-p: the same for the p-frame size probe (pfv_enc_probe_pframe_dev: k_probe_pframe + k_pprobe_sizes), frame 1 of the synthetic streams
behind frame 0 as an i-frame at the middle rung.  B = per rung pfv_enc_pframe_dev + pfv_enc_pack_pframe_dev to the size (payload capacity 24);
a p-frame encode moves prev_frame, so every rung of B starts from a fresh i-frame that is enqueued OUTSIDE its event pair, and B is the sum of
the rungs' pairs.  Sizes against trial encodes from the same prev_frame at every rung of all streams; then the host clock around pfv_encoder:
encode_pframe with the hard budget off / on, and encode_frame against encode_pframe.

--probe-rd: the i-frame rate-distortion probe (pfv_encoder_probe_iframe_rd) on the clip's first frame -- probed against written payload bytes
and probed against reported squared error per rung -- and then its timing at 96 x 1080p, ladders 0,2,5,7,10 and 0..10, by --probe's method:
A = the probe's two launches (k_probe_iframe_rd + k_probe_rd_sizes); B = the way to the same numbers without it, per rung
pfv_enc_session_set_rung + pfv_enc_iframe_dev + the entropy stage to the size + pfv_enc_distortion_dev; C = pfv_enc_probe_iframe_dev alone
(what the distortion half adds is A - C).  The answers are compared rung by rung over all streams.

--probe-p-rd: the p-frame rate-distortion probe (pfv_encoder_probe_pframe_rd) on the clip's second frame behind its first -- probed against
written payload bytes and reported squared error per rung -- and then its timing at 96 x 1080p by --probe-p's method: A = the probe's two
launches (k_probe_pframe_rd + k_pprobe_rd_sizes); B = per rung pfv_enc_session_set_rung + pfv_enc_pframe_dev + pfv_enc_pack_pframe_dev to the
size + pfv_enc_distortion_dev, the i-frame that restores prev_frame enqueued outside the rung's event pair; C = pfv_enc_probe_pframe_dev alone.
Sizes and plane sums against the trial encodes at every rung of all streams; then the host clock around pfv_encoder: encode_pframe and
encode_frame with the p-frame quality floor off / on.

--probe-ssim / --probe-p-ssim: the SSIM probes (pfv_encoder_probe_iframe_ssim on the clip's first frame / pfv_encoder_probe_pframe_ssim on its
second frame behind the first) -- probed against written payload bytes, reported squared error and reported SSIM sums per rung -- and then
their timing at 96 x 1080p, ladders 0,2,5,7,10 and 0..10, by the methods above: A = the probe's three launches (k_probe_iframe_ssim or
k_probe_pframe_ssim, k_probe_ssim_windows, the RD probe's tail); B = per rung the trial encode to the size + pfv_enc_distortion_dev +
pfv_enc_ssim_dev; C = the RD probe of the same frame type (what the SSIM half adds is A - C).  Sizes, plane sums and SSIM sums against the
trial encodes at every rung of all streams; the bytes of the block-sum map.
--time-scale (on the GPU box) adds thirteen lines: k_scale on 96 x 1080p frames in HBM -> 720p, -> 540p, -> 240x136 and 540p -> 1080p, each for
the three kinds, against the bytes it must move (source read once plus destination written once), and pfv_dec_get_frame_dev (k_crop_frames) on
the same frames as the streaming yardstick; "rate_over_crop_rate" is the fraction of its byte rate.  Method and the PFV_HIP_LIB rule as
--time-present (with PFV_HIP_LIB: one WIDTH x HEIGHT stream, the rows only).
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


def encode_clip(pkg, ctx, w, h, n_frames, gop, kind, quality, frame_report=True, ssim_out=None):
    """-> (stream bytes, reports, seconds per encode call); ssim_out: a list that receives the FrameSsim of every frame"""
    st = pkg.SyntheticStream(w, h, kind=kind)
    buf = io.BytesIO()
    enc = pkg.Encoder(buf, w, h, 30, quality, ctx, frame_report=frame_report, frame_ssim=ssim_out is not None)
    reports, secs = [], []
    for t in range(n_frames):
        fr = pkg.VideoFrame.from_packed(w, h, st.frame(t))
        t0 = time.perf_counter()
        (enc.encode_iframe if t % gop == 0 else enc.encode_pframe)(fr)
        secs.append(time.perf_counter() - t0)
        if frame_report:
            reports.append(enc.last_report)
        if ssim_out is not None:
            ssim_out.append(enc.last_ssim)
    enc.finish()
    enc.close()
    return buf.getvalue(), reports, secs


def rd_line(pkg, ctx, w, h, n_frames, gop, kind, quality, with_ssim=False):
    ssims = [] if with_ssim else None
    data, reports, _ = encode_clip(pkg, ctx, w, h, n_frames, gop, kind, quality, ssim_out=ssims)
    by = {1: [r.packet_bytes for r in reports if r.type == 1], 2: [r.packet_bytes for r in reports if r.type == 2]}
    mean = lambda v: float(sum(v) / len(v)) if v else None   # noqa: E731
    line = {"quality": quality, "width": w, "height": h, "frames": n_frames, "gop": gop, "kind": kind,
            "stream_bytes": len(data), "packet_bytes": sum(r.packet_bytes for r in reports),
            "bytes_per_frame": mean([r.packet_bytes for r in reports]),
            "iframes": len(by[1]), "iframe_bytes_per_frame": mean(by[1]), "pframes": len(by[2]), "pframe_bytes_per_frame": mean(by[2]),
            "psnr_y": mean([r.psnr[0] for r in reports]), "psnr_u": mean([r.psnr[1] for r in reports]),
            "psnr_v": mean([r.psnr[2] for r in reports]), "psnr_yuv": mean([r.psnr_yuv for r in reports])}
    if with_ssim:
        line.update({"ssim_y": mean([r.ssim[0] for r in ssims]), "ssim_u": mean([r.ssim[1] for r in ssims]),
                     "ssim_v": mean([r.ssim[2] for r in ssims]), "ssim_all": mean([r.ssim_all for r in ssims])})
    return line


def time_ssim(pkg, ctx, n_streams=96, w=1920, h=1080, warmup=5, samples=30):
    lib = ctx._lib
    fb = int(lib.pfv_frame_bytes(w, h))
    tb = int(lib.pfv_total_blocks(w, h))
    frames = ctx.alloc(fb * n_streams)
    coef = ctx.alloc(n_streams * tb * 512)
    sums = ctx.alloc(n_streams * 24)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, frames)
    enc = pkg.EncoderSession(ctx, w, h, 5, n_streams)
    enc.encode_iframe_dev(frames, coef)           # prev_frame = the reconstruction of `frames`
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()

    def mean_ms(fn):
        got = []
        for k in range(warmup + samples):
            ctx.record(e0)
            fn()
            ctx.record(e1)
            ms = ctypes.c_float()
            ctx.check(lib.pfv_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            if k >= warmup:
                got.append(float(ms.value))
        return statistics.mean(got), min(got), max(got)
    # alternate the two, so that whatever else the box is doing meets both
    res = {"ssim": [], "sse": []}
    for _ in range(3):
        res["ssim"].append(mean_ms(lambda: enc.ssim_dev(frames, sums)))
        res["sse"].append(mean_ms(lambda: enc.distortion_dev(frames, sums)))
    q24 = np.zeros((n_streams, 3), dtype=np.int64)
    enc.ssim_dev(frames, sums)
    ctx.download(q24, sums)
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    enc.close()
    for p in (frames, coef, sums):
        ctx.free(p)
    ssim_ms = statistics.mean(m for m, _, _ in res["ssim"])
    sse_ms = statistics.mean(m for m, _, _ in res["sse"])
    bytes_moved = n_streams * (fb + int(lib.pfv_padded_frame_bytes(w, h)))     # both operands once; the halo rows and columns are re-reads
    nw = pkg.ssim_windows(w, h)
    return {"shape": f"{n_streams} x {w}x{h}", "samples_per_round": samples, "rounds": 3, "ssim_pair_ms": ssim_ms, "sse_pair_ms": sse_ms,
            "ratio": ssim_ms / sse_ms, "ssim_rounds_ms": res["ssim"], "sse_rounds_ms": res["sse"], "operand_bytes_per_launch": bytes_moved,
            "ssim_GBps": bytes_moved / ssim_ms / 1e6, "sse_GBps": bytes_moved / sse_ms / 1e6,
            "ssim_all_stream0": pkg.ssim(int(q24[0].sum()), sum(nw))}


def deblock_line(pkg, ctx, w, h, n_frames, gop, kind, quality, dump=None):
    """the keys --deblock adds to a quality's line"""
    lib = ctx._lib
    P = ctypes.c_void_p
    fb, tb = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h))
    tabs = pkg.qtables_from_quality(quality)[:4]
    s = [pkg.deblock_strength(t) for t in tabs]
    strength = {True: np.array([s[0], s[1], s[1]], np.uint8), False: np.array([s[2], s[3], s[3]], np.uint8)}     # i-frame / p-frame tables
    st = pkg.SyntheticStream(w, h, kind=kind)
    enc = pkg.EncoderSession(ctx, w, h, quality, 1)
    bufs = [ctx.alloc(n) for n in (fb, tb * 512, tb * 2, tb, fb, 24, 24)]
    frame_d, coef_d, mv_d, has_d, out_d, sse_d, ssim_d = bufs
    nw = pkg.ssim_windows(w, h)
    dims = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    rows = {"plain": [], "db": []}
    dumped = {"input": [], "recon": [], "deblocked": []}
    try:
        for t in range(n_frames):
            f = st.frame(t)
            ctx.upload(frame_d, f)
            intra = t % gop == 0
            if intra:
                enc.encode_iframe_dev(frame_d, coef_d)
            else:
                enc.encode_pframe_dev(frame_d, mv_d, has_d, coef_d)
            prev = lib.pfv_enc_prev_frame_dev(enc.handle, 0)
            ctx.check(lib.pfv_frames_deblock_dev(ctx.handle, w, h, 1, P(prev), pkg._lib.PFV_FRAME_PADDED, 0, P(out_d), 0, strength[intra].ctypes.data_as(P)))
            for key, b_dev, layout in (("plain", prev, pkg._lib.PFV_FRAME_PADDED), ("db", out_d, pkg._lib.PFV_FRAME_PACKED)):
                ctx.check(lib.pfv_frames_sse_dev(ctx.handle, w, h, 1, P(frame_d), pkg._lib.PFV_FRAME_PACKED, 0, P(b_dev), layout, 0, P(sse_d), None))
                ctx.check(lib.pfv_frames_ssim_dev(ctx.handle, w, h, 1, P(frame_d), pkg._lib.PFV_FRAME_PACKED, 0, P(b_dev), layout, 0, P(ssim_d), None))
                sse, q24 = np.zeros(3, np.uint64), np.zeros(3, np.int64)
                ctx.download(sse, sse_d)
                ctx.download(q24, ssim_d)
                rows[key].append([pkg.psnr(int(sse[i]), dims[i][0] * dims[i][1]) for i in range(3)] + [pkg.psnr(int(sse.sum()), fb)] +
                                 [pkg.ssim(int(q24[i]), nw[i]) for i in range(3)] + [pkg.ssim(int(q24.sum()), sum(nw))])
            if dump:
                got = np.zeros(fb, np.uint8)
                ctx.download(got, out_d)
                pad = enc.prev_frame()[0]
                parts, off = [], 0
                for pw, ph in dims:
                    sw, sh = (pw + 15) // 16 * 16, (ph + 15) // 16 * 16
                    parts.append(pad[off:off + sw * sh].reshape(sh, sw)[:ph, :pw].reshape(-1))
                    off += sw * sh
                dumped["input"].append(f); dumped["recon"].append(np.concatenate(parts)); dumped["deblocked"].append(got)
    finally:
        enc.close()
        for b in bufs:
            ctx.free(b)
    if dump:
        os.makedirs(dump, exist_ok=True)
        for name, frames in dumped.items():
            np.concatenate(frames).tofile(os.path.join(dump, f"q{quality}_{name}.yuv"))
    names = ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "ssim_y", "ssim_u", "ssim_v", "ssim_all")
    line = {"db_strength_i": [int(v) for v in strength[True]], "db_strength_p": [int(v) for v in strength[False]]}
    for k, name in enumerate(names):
        if name.startswith("ssim"):
            line[name] = float(sum(r[k] for r in rows["plain"]) / len(rows["plain"]))
        line["db_" + name] = float(sum(r[k] for r in rows["db"]) / len(rows["db"]))
    return line


def time_deblock(pkg, ctx, n_streams=96, w=1920, h=1080, warmup=5, samples=30):
    lib = ctx._lib
    fb, tb = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h))
    f0, f1, out = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    coef, mv, has = ctx.alloc(n_streams * tb * 512), ctx.alloc(n_streams * tb * 2), ctx.alloc(n_streams * tb)
    seeds = np.arange(1, n_streams + 1, dtype=np.uint64)
    ctx.synth_frames_dev(w, h, seeds, 0, f0)
    ctx.synth_frames_dev(w, h, seeds, 1, f1)
    enc = pkg.EncoderSession(ctx, w, h, 10, n_streams)
    dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(10)[:4]), n_streams)
    enc.encode_iframe_dev(f0, coef)
    dec.decode_iframe_dev(coef)                   # framebuffer = frame 0 at quality 10: the blocking the filter is for
    enc.encode_pframe_dev(f1, mv, has, coef)
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
    modes = {"deblock": ("fixed", (5, 10, 10)), "deblock_s0": ("fixed", (0, 0, 0)), "crop": ("off", None)}
    res = {k: [] for k in modes}
    for _ in range(3):                            # alternate, so that whatever else the box is doing meets all of them
        for key, (mode, st) in modes.items():
            dec.set_deblock(mode, st)
            res[key].append(median_ms(lambda: dec.get_frame_dev(out)))
    loop = {"off": [], "auto": []}
    dec.set_output_dev(out)
    for _ in range(3):
        for mode in loop:
            dec.set_deblock(mode)
            loop[mode].append(median_ms(lambda: dec.decode_pframe_dev(mv, has, coef)))
    ctx.sync()
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    enc.close(); dec.close()
    for p in (f0, f1, out, coef, mv, has):
        ctx.free(p)
    med = {k: statistics.median(m for m, _, _ in v) for k, v in res.items()}
    bytes_moved = n_streams * (fb + int(lib.pfv_padded_frame_bytes(w, h)))
    return {"shape": f"{n_streams} x {w}x{h}", "samples_per_round": samples, "rounds": 3, "deblock_ms": med["deblock"], "deblock_s0_ms": med["deblock_s0"],
            "crop_ms": med["crop"], "ratio": med["deblock"] / med["crop"], "ratio_s0": med["deblock_s0"] / med["crop"], "rounds_ms": res,
            "bytes_per_launch": bytes_moved, "deblock_GBps": bytes_moved / med["deblock"] / 1e6, "crop_GBps": bytes_moved / med["crop"] / 1e6,
            "dec_pframe_plus_output_off_ms": statistics.median(m for m, _, _ in loop["off"]),
            "dec_pframe_plus_output_auto_ms": statistics.median(m for m, _, _ in loop["auto"]), "dec_pframe_rounds_ms": loop}


def noisy_clip(pkg, w, h, n_frames, kind, seed=2024):
    """the synthetic clip and the same clip with seeded uniform noise in [-3, 3], clipped"""
    st = pkg.SyntheticStream(w, h, kind=kind)
    clean = np.stack([st.frame(t) for t in range(n_frames)])
    rng = np.random.default_rng(seed)
    return clean, np.clip(clean.astype(np.int64) + rng.integers(-3, 4, clean.shape), 0, 255).astype(np.uint8)


def denoise_line(pkg, ctx, w, h, n_frames, gop, kind, quality, ss, st, dump=None):
    """the keys --denoise adds to a quality's line: the NOISY clip encoded without and with the pre-filter (pfv_encoder_set_denoise)"""
    clean, noisy = noisy_clip(pkg, w, h, n_frames, kind)
    spatial, temporal = (ss,) * 3, (st,) * 3
    filt = pkg.frames_denoise(ctx, w, h, noisy, spatial, temporal)
    out = {"dn_strength": [ss, st]}
    for key, on in (("noisy", False), ("dn", True)):
        buf = io.BytesIO()
        enc = pkg.Encoder(buf, w, h, 30, quality, ctx)
        sess = pkg.EncoderSession(ctx, w, h, quality, 1)
        if on:
            enc.set_denoise(True, spatial, temporal)
        skipped = total = 0
        for t in range(n_frames):
            (enc.encode_iframe if t % gop == 0 else enc.encode_pframe)(pkg.VideoFrame.from_packed(w, h, noisy[t]))
            f = filt[t] if on else noisy[t]
            if t % gop == 0:
                sess.encode_iframe(f)
            else:
                _, has, _ = sess.encode_pframe(f)
                skipped, total = skipped + int((has == 0).sum()), total + int(has.size)
        enc.finish()
        enc.close()
        sess.close()
        d = (clean.astype(np.int64) - (filt if on else noisy)) ** 2
        out.update({f"{key}_stream_bytes": len(buf.getvalue()), f"{key}_bytes_per_frame": len(buf.getvalue()) / n_frames,
                    f"{key}_psnr_clean": pkg.psnr(int(d.sum()), d.size), f"{key}_skipped": skipped, f"{key}_skipped_share": skipped / total if total else None})
    out["pframe_macroblocks"] = total
    if dump:
        os.makedirs(dump, exist_ok=True)
        for name, arr in (("clean", clean), ("noisy", noisy), ("denoised", filt)):
            arr.tofile(os.path.join(dump, f"q{quality}_{name}.yuv"))
    return out


def time_denoise(pkg, ctx, n_streams=96, w=1920, h=1080, warmup=5, samples=30, rounds=3):
    """k_denoise (committed, strengths 6 / 6, packed and padded source) beside k_deblock (padded source, strengths 5 / 10 / 10) and k_crop_frames
    on the same frames: medians of HIP-event times on the context's stream, the kernels alternating in every round"""
    lib = ctx._lib
    P = ctypes.c_void_p
    fb, tb = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h))
    f0, out = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    coef = ctx.alloc(n_streams * tb * 512)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, f0)
    enc = pkg.EncoderSession(ctx, w, h, 10, n_streams)
    dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(10)[:4]), n_streams)
    enc.encode_iframe_dev(f0, coef)
    dec.decode_iframe_dev(coef)
    prev = lib.pfv_enc_prev_frame_dev(enc.handle, 0)          # the same frames, padded
    dn = pkg.Denoiser(ctx, w, h, n_streams, (6, 6, 6), (6, 6, 6))
    dn.run_dev(f0, out)                                        # primes: the timed runs are the steady state, one kernel each
    st = np.array([5, 10, 10], np.uint8)
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
        return statistics.median(got)
    dec.set_deblock("off")
    cases = {"denoise_packed": lambda: dn.run_dev(f0, out), "denoise_padded": lambda: dn.run_dev(prev, out, src_layout="padded"),
             "deblock": lambda: ctx.check(lib.pfv_frames_deblock_dev(ctx.handle, w, h, n_streams, P(prev), pkg._lib.PFV_FRAME_PADDED, 0, P(out), 0, st.ctypes.data_as(P))),
             "crop": lambda: dec.get_frame_dev(out)}
    res = {k: [] for k in cases}
    for _ in range(rounds):                       # alternate, so that whatever else the box is doing meets all of them
        for key, fn in cases.items():
            res[key].append(median_ms(fn))
    ctx.sync()
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    dn.close(); enc.close(); dec.close()
    for p in (f0, out, coef):
        ctx.free(p)
    med = {k: statistics.median(v) for k, v in res.items()}
    pfb = int(lib.pfv_padded_frame_bytes(w, h))
    moved = {"denoise_packed": n_streams * 4 * fb, "denoise_padded": n_streams * (pfb + 3 * fb), "deblock": n_streams * (pfb + fb), "crop": n_streams * (pfb + fb)}
    return {"shape": f"{n_streams} x {w}x{h}", "samples_per_round": samples, "rounds": rounds, **{f"{k}_ms": v for k, v in med.items()},
            **{f"{k}_GBps": moved[k] / med[k] / 1e6 if med[k] else None for k in med}, "rounds_ms": res}


def scene_cut_line(pkg, ctx, w, h, n_frames, quality, threshold, radius, max_interval=15):
    """a clip spliced from SyntheticStream(SEED, "pan") and SyntheticStream(SEED + 17, "low_motion") in segments, encoded twice through
    pfv_encoder with explicit frame types: an i-frame every `max_interval` frames, and the types pfv_scene_plan makes of the detector's stats
    (min_interval 1, the same max_interval).  Bytes and worst-frame PSNR-YUV from the frame reports."""
    from pretty_fast_video_amd.synth import SEED
    segment = 11 if n_frames >= 22 else max(3, n_frames // 3)
    a, b = pkg.SyntheticStream(w, h, seed=SEED, kind="pan"), pkg.SyntheticStream(w, h, seed=SEED + 17, kind="low_motion")
    clip = np.stack([(b if (t // segment) % 2 else a).frame(t) for t in range(n_frames)])
    stats = pkg.frames_scene(ctx, w, h, clip, radius).reshape(-1)
    scores = [pkg.scene_score(s) for s in stats]
    planned = pkg.scene_plan(stats, threshold, 1, max_interval).tolist()
    fixed = [1 if t % max_interval == 0 else 2 for t in range(n_frames)]
    line = {"threshold_q8": threshold, "radius": radius, "quality": quality, "width": w, "height": h, "frames": n_frames, "segment": segment,
            "splices": [t for t in range(1, n_frames) if t % segment == 0], "scores_q8": scores, "planned_types": planned, "fixed_types": fixed}
    for name, types in (("planned", planned), ("fixed", fixed)):
        enc = pkg.Encoder(io.BytesIO(), w, h, 30, quality, ctx, frame_report=True)
        reports = []
        for ty, f in zip(types, clip):
            (enc.encode_iframe if ty == 1 else enc.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
            reports.append(enc.last_report)
        enc.finish()
        enc.close()
        line.update({f"{name}_bytes": sum(r.packet_bytes for r in reports), f"{name}_iframes": types.count(1),
                     f"{name}_worst_psnr": min(r.psnr_yuv for r in reports), f"{name}_mean_psnr": float(sum(r.psnr_yuv for r in reports) / len(reports))})
    return line


def time_scene(pkg, ctx, n_streams=96, w=1920, h=1080, clip=(3840, 2160, 60), quality=5, warmup=5, samples=30, rounds=3):
    """the three scene kernels at n_streams x w x h (run_dev, uncommitted, R = 4 and R = 7) and on one clip (run_clip_dev, R = 4): per kernel from
    the events pfv_scene_detector_run_timed_dev records between them, per launch group from an event pair around run_dev / run_clip_dev; beside
    them k_sse_mb + k_sse_sum on the same two frames and the default p-frame encode.  Medians, the cases alternating in every round."""
    lib = ctx._lib
    P = ctypes.c_void_p
    fb, tb = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h))
    f0, f1 = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    coef, mv, has = ctx.alloc(n_streams * tb * 512), ctx.alloc(n_streams * tb * 2), ctx.alloc(n_streams * tb)
    cw, ch, cn = clip
    cfb = int(lib.pfv_frame_bytes(cw, ch))
    frames = ctx.alloc(cfb * cn)
    stats, sse = ctx.alloc(40 * max(n_streams, cn)), ctx.alloc(8 * 3 * n_streams)
    seeds = np.arange(1, n_streams + 1, dtype=np.uint64)
    ctx.synth_frames_dev(w, h, seeds, 0, f0)
    ctx.synth_frames_dev(w, h, seeds, 1, f1)
    for t in range(cn):
        ctx.synth_frames_dev(cw, ch, seeds[:1], t, frames + t * cfb)
    enc = pkg.EncoderSession(ctx, w, h, quality, n_streams)
    det = pkg.SceneDetector(ctx, w, h, n_streams)
    cdet = pkg.SceneDetector(ctx, cw, ch, 1, max_clip_frames=cn)
    det.run_dev(f0, stats)                                     # primes: the timed runs are the steady state
    cdet.run_clip_dev(frames, 1, stats)
    ctx.check(lib.pfv_frames_sse_dev(ctx.handle, w, h, n_streams, P(f0), 0, 0, P(f1), 0, 0, P(sse), None))      # makes the map scratch
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()

    def median_ms(fn, before=None):
        got = []
        for k in range(warmup + samples):
            if before:
                before()
            ctx.record(e0)
            fn()
            ctx.record(e1)
            ms = ctypes.c_float()
            ctx.check(lib.pfv_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            if k >= warmup:
                got.append(float(ms.value))
        return statistics.median(got)

    def kernels_ms(d, src, n, radius, is_clip):
        d.set_radius(radius)
        got = [d.run_timed_dev(src, n, stats, clip=is_clip) for _ in range(warmup + samples)][warmup:]
        return [statistics.median(g_[i] for g_ in got) for i in range(3)]

    def group(d, radius, fn):
        d.set_radius(radius)
        return median_ms(fn)
    cases = {
        "run_dev_r4": lambda: group(det, 4, lambda: det.run_dev(f1, stats, commit=False)),
        "run_dev_r7": lambda: group(det, 7, lambda: det.run_dev(f1, stats, commit=False)),
        "run_clip_dev_r4": lambda: group(cdet, 4, lambda: cdet.run_clip_dev(frames, cn, stats, commit=False)),
        "sse_pair": lambda: median_ms(lambda: ctx.check(lib.pfv_frames_sse_dev(ctx.handle, w, h, n_streams, P(f0), 0, 0, P(f1), 0, 0, P(sse), None))),
        "enc_pframe": lambda: median_ms(lambda: enc.encode_pframe_dev(f1, mv, has, coef), before=lambda: enc.encode_iframe_dev(f0, coef)),
    }
    res = {k: [] for k in cases}
    stages = {"r4": [], "r7": [], "clip_r4": []}
    for _ in range(rounds):                       # alternate, so that whatever else the box is doing meets all of them
        for key, fn in cases.items():
            res[key].append(fn())
        stages["r4"].append(kernels_ms(det, f1, n_streams, 4, False))
        stages["r7"].append(kernels_ms(det, f1, n_streams, 7, False))
        stages["clip_r4"].append(kernels_ms(cdet, frames, cn, 4, True))
    ctx.sync()
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    det.close(); cdet.close(); enc.close()
    for p in (f0, f1, coef, mv, has, frames, stats, sse):
        ctx.free(p)
    med = {k: statistics.median(v) for k, v in res.items()}
    st = {k: [statistics.median(x[i] for x in v) for i in range(3)] for k, v in stages.items()}
    over = lambda x, y: x / y if y else None      # noqa: E731  (an emulated device has no clock: its events are 0 ms apart)
    blocks = n_streams * ((w >> 2) >> 3) * ((h >> 2) >> 3)
    return {"shape": f"{n_streams} x {w}x{h}", "clip": f"{cn} x {cw}x{ch}", "samples_per_round": samples, "rounds": rounds,
            "quarter_ms": st["r4"][0], "cost_r4_ms": st["r4"][1], "cost_r7_ms": st["r7"][1], "sum_ms": st["r4"][2],
            "clip_quarter_ms": st["clip_r4"][0], "clip_cost_r4_ms": st["clip_r4"][1], "clip_sum_ms": st["clip_r4"][2],
            **{f"{k}_ms": v for k, v in med.items()},
            "quarter_GBps": over(n_streams * (w * h + (w >> 2) * (h >> 2)) / 1e6, st["r4"][0]),
            "cost_r4_ns_per_block": over(st["r4"][1] * 1e6, blocks), "cost_r7_ns_per_block": over(st["r7"][1] * 1e6, blocks),
            "run_dev_r4_over_enc_pframe": over(med["run_dev_r4"], med["enc_pframe"]), "run_dev_r4_over_sse_pair": over(med["run_dev_r4"], med["sse_pair"]),
            "blocks": blocks, "rounds_ms": res}


def pan_clip(w, h, n_frames, dx, dy, seed=7):
    """packed frames of a smoothed random canvas seen through a window that moves by (dx, dy) per frame; chroma is the luma at the even positions"""
    rng = np.random.default_rng(seed)
    mx, my = abs(dx) * (n_frames - 1), abs(dy) * (n_frames - 1)
    c = rng.integers(0, 256, (h + my + 2, w + mx + 2)).astype(np.int32)
    c = (c[:-2, :-2] + c[1:-1, :-2] + c[2:, :-2] + c[:-2, 1:-1] + 2 * c[1:-1, 1:-1] + c[2:, 1:-1] + c[:-2, 2:] + c[1:-1, 2:] + c[2:, 2:]) // 10
    c = np.clip((c - 128) * 3 + 128, 0, 255).astype(np.uint8)
    out = []
    for t in range(n_frames):
        ox, oy = (t * dx if dx >= 0 else mx + t * dx), (t * dy if dy >= 0 else my + t * dy)
        y = c[oy:oy + h, ox:ox + w]
        u = y[::2, ::2][:h // 2, :w // 2]
        out.append(np.concatenate([y.reshape(-1), u.reshape(-1), (255 - u).reshape(-1)]))
    return out


def search_line(pkg, ctx, w, h, n_frames, gop, kind, quality, radius, mode="full", pan=None):
    """the keys --search adds to a quality's line: the clip under the four-step search and under `mode` at `radius` ("hier": and under the
    exhaustive search at radius 15)"""
    if pan:
        clip = pan_clip(w, h, n_frames, *pan)
    else:
        st = pkg.SyntheticStream(w, h, kind=kind)
        clip = [st.frame(t) for t in range(n_frames)]
    out = {"search_radius": radius}
    if pan:
        out["search_pan"] = list(pan)
    cases = (("four", "fourstep", 0), ("full", "full", radius)) if mode == "full" else (("four", "fourstep", 0), ("full", "full", 15), ("hier", "hier", radius))
    for key, m, r in cases:
        buf = io.BytesIO()
        enc = pkg.Encoder(buf, w, h, 30, quality, ctx, frame_report=True)
        sess = pkg.EncoderSession(ctx, w, h, quality, 1)
        enc.set_motion_search(m, r)
        sess.set_motion_search(m, r)
        coded = skipped = 0
        psnr = []
        for t, f in enumerate(clip):
            (enc.encode_iframe if t % gop == 0 else enc.encode_pframe)(pkg.VideoFrame.from_packed(w, h, f))
            psnr.append(enc.last_report.psnr_yuv)
            if t % gop == 0:
                sess.encode_iframe(f)
            else:
                _, has, _ = sess.encode_pframe(f)
                coded, skipped = coded + int((has != 0).sum()), skipped + int((has == 0).sum())
        enc.finish()
        enc.close()
        sess.close()
        out.update({f"{key}_stream_bytes": len(buf.getvalue()), f"{key}_psnr_yuv": float(sum(psnr) / len(psnr)), f"{key}_coded": coded, f"{key}_skipped": skipped})
    return out


def time_search(pkg, ctx, n_streams=96, w=1920, h=1080, quality=5, warmup=5, samples=30, rounds=3):
    """pfv_enc_pframe_dev of frame 1 behind frame 0 as an i-frame: the default p-frame encode against PFV_SEARCH_FULL at R = 7 and R = 15 (two
    launches each: k_pf_search_full + k_pf_transform).  A p-frame encode moves prev_frame: the i-frame that restores it is enqueued OUTSIDE the
    event pair.  Medians of HIP-event times on the context's stream, the three alternating in every round"""
    lib = ctx._lib
    fb, tb = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h))
    f0, f1 = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    coef, mv, has = ctx.alloc(n_streams * tb * 512), ctx.alloc(n_streams * tb * 2), ctx.alloc(n_streams * tb)
    seeds = np.arange(1, n_streams + 1, dtype=np.uint64)
    ctx.synth_frames_dev(w, h, seeds, 0, f0)
    ctx.synth_frames_dev(w, h, seeds, 1, f1)
    enc = pkg.EncoderSession(ctx, w, h, quality, n_streams)
    e0, e1 = ctx.event(), ctx.event()

    def median_ms(mode, radius):
        enc.set_motion_search(mode, radius)
        got, coded = [], 0
        for k in range(warmup + samples):
            enc.encode_iframe_dev(f0, coef)
            ctx.record(e0)
            enc.encode_pframe_dev(f1, mv, has, coef)
            ctx.record(e1)
            ms = ctypes.c_float()
            ctx.check(lib.pfv_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            if k >= warmup:
                got.append(float(ms.value))
        flags = np.zeros(n_streams * tb, np.uint8)
        ctx.download(flags, has)
        return statistics.median(got), int(flags.sum())
    def stages_ms(radius):
        enc.set_motion_search("hier", radius)
        got = []
        for k in range(warmup + samples):
            enc.encode_iframe_dev(f0, coef)
            st = enc.encode_pframe_hier_timed_dev(f1, mv, has, coef)
            if k >= warmup:
                got.append(st)
        return {name: statistics.median(g_[name] for g_ in got) for name in enc.HIER_STAGES}
    cases = {"fourstep": ("fourstep", 0), "full_r7": ("full", 7), "full_r15": ("full", 15), "hier_r30": ("hier", 30), "hier_r62": ("hier", 62)}
    res, coded, stages = {k: [] for k in cases}, {}, {"hier_r30": [], "hier_r62": []}
    for _ in range(rounds):                       # alternate, so that whatever else the box is doing meets all of them
        for key, (mode, radius) in cases.items():
            ms, coded[key] = median_ms(mode, radius)
            res[key].append(ms)
            if mode == "hier":
                stages[key].append(stages_ms(radius))
    ctx.sync()
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    enc_stages = enc.HIER_STAGES
    enc.close()
    for p in (f0, f1, coef, mv, has):
        ctx.free(p)
    med = {k: statistics.median(v) for k, v in res.items()}
    # the products alone: (2R + 1)^2 candidates x 64 v_dot4 per macroblock, spread over its 8 lanes = (2R + 1)^2 x 8 wave-instructions per
    # wavefront of 8 macroblocks (partial strips make the wavefronts a few more than macroblocks / 8)
    waves = n_streams * int(lib.pfv_total_blocks(w, h)) / 8.0
    floor = {k: waves * (2 * r + 1) ** 2 * 8 * 4.2 / 1024 / 2.4e9 * 1e3 for k, (m_, r) in cases.items() if m_ == "full"}
    # the coarse level: (2 Rc + 1)^2 candidates x 16 v_dot4 per macroblock over its 8 lanes
    cfloor = {k: waves * (r + 1) ** 2 * 2 * 4.2 / 1024 / 2.4e9 * 1e3 for k, (m_, r) in cases.items() if m_ == "hier"}
    hier = {f"{k}_stages_ms": {n: statistics.median(x[n] for x in v) for n in enc_stages} for k, v in stages.items()}
    hier.update({f"{k}_coarse_dot4_floor_ms": v for k, v in cfloor.items()})
    hier.update({f"{k}_coarse_over_floor": (hier[f"{k}_stages_ms"]["coarse"] / v if hier[f"{k}_stages_ms"]["coarse"] else None) for k, v in cfloor.items()})
    over = lambda x, y: x / y if y else None      # noqa: E731  (an emulated device has no clock: its events are 0 ms apart)
    return {"shape": f"{n_streams} x {w}x{h}", "streams": n_streams, "quality": quality, "samples_per_round": samples, "rounds": rounds,
            **{f"{k}_ms": v for k, v in med.items()}, **{f"{k}_over_fourstep": over(med[k], med["fourstep"]) for k in floor},
            **{f"{k}_dot4_floor_ms": v for k, v in floor.items()}, **{f"{k}_over_floor": over(med[k], floor[k]) for k in floor},
            **hier, "coded_macroblocks": coded, "macroblocks": n_streams * tb, "rounds_ms": res}


def time_present(pkg, ctx, fmt, n_streams=96, w=1920, h=1080, warmup=5, samples=30, rounds=3):
    lib = ctx._lib
    fb, tb = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h))
    bpp = int(lib.pfv_rgb_row_bytes(w, pkg.quality.pix_format(fmt))) // w
    f0, planar, coef = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams), ctx.alloc(n_streams * tb * 512)
    rgb, rgb3 = ctx.alloc(w * h * bpp * n_streams), ctx.alloc(w * h * 3 * n_streams)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, f0)
    enc = pkg.EncoderSession(ctx, w, h, 5, n_streams)
    dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(5)[:4]), n_streams)
    enc.encode_iframe_dev(f0, coef)
    dec.decode_iframe_dev(coef)                   # the framebuffer holds decoded pictures
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

    def without():                                # the crop, then one launch per stream: RGB8 whatever `fmt` is
        dec.get_frame_dev(planar)
        for k in range(n_streams):
            ctx.check(lib.pfv_yuv420_to_rgb_dev(ctx.handle, ctypes.c_void_p(planar + k * fb), w, h, ctypes.c_void_p(rgb3 + k * w * h * 3)))
    ways = {"a_present": lambda: dec.get_frame_rgb_dev(rgb, fmt), "b_crop_plus_per_stream": without, "c_crop": lambda: dec.get_frame_dev(planar)}
    res = {k: [] for k in ways}
    for _ in range(rounds):                       # alternate, so that whatever else the box is doing meets all of them
        for key, fn in ways.items():
            res[key].append(median_ms(fn))
    ctx.sync()
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    enc.close(); dec.close()
    for p in (f0, planar, coef, rgb, rgb3):
        ctx.free(p)
    med = {k: statistics.median(m for m, _, _ in v) for k, v in res.items()}
    moved = {"a_present": n_streams * (fb + w * h * bpp), "b_crop_plus_per_stream": n_streams * (2 * fb + fb + w * h * 3), "c_crop": n_streams * 2 * fb}
    over = lambda x, y: x / y if y else None      # noqa: E731  (an emulated device has no clock: its events are 0 ms apart)
    gbps = {k: over(moved[k], med[k] * 1e6) for k in ways}
    return {"shape": f"{n_streams} x {w}x{h}", "format": fmt, "samples_per_round": samples, "rounds": rounds,
            "a_present_ms": med["a_present"], "b_crop_plus_per_stream_ms": med["b_crop_plus_per_stream"], "c_crop_ms": med["c_crop"],
            "bytes": moved, "GBps": gbps, "a_over_b_time": over(med["a_present"], med["b_crop_plus_per_stream"]),
            "a_rate_over_c_rate": over(gbps["a_present"], gbps["c_crop"]) if gbps["a_present"] else None, "rounds_ms": res}


def scale_cases(w, h):
    """the four size pairs of --time-scale for a w x h frame: down to 2/3, 1/2 and 1/8 (sizes rounded up to even), and w/2 x h/2 up to w x h"""
    ev = lambda n, num, den: ((n * num + den - 1) // den + 1) // 2 * 2      # noqa: E731
    return [(w, h, ev(w, 2, 3), ev(h, 2, 3)), (w, h, ev(w, 1, 2), ev(h, 1, 2)), (w, h, ev(w, 1, 8), ev(h, 1, 8)), (ev(w, 1, 2), ev(h, 1, 2), w, h)]


def time_scale(pkg, ctx, n_streams=96, w=1920, h=1080, warmup=5, samples=30, rounds=3):
    """k_scale (pfv_scaler_run_dev, packed frames in HBM) per size pair and kind, and pfv_dec_get_frame_dev (k_crop_frames) of n_streams w x h
    frames as the streaming yardstick: medians of HIP-event times after warm-up, the ways alternated per round"""
    lib = ctx._lib
    fb, tb = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h))
    f0, planar, coef = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams), ctx.alloc(n_streams * tb * 512)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, f0)
    enc = pkg.EncoderSession(ctx, w, h, 5, n_streams)
    dec = pkg.DecoderSession(ctx, w, h, np.stack(pkg.qtables_from_quality(5)[:4]), n_streams)
    enc.encode_iframe_dev(f0, coef)
    dec.decode_iframe_dev(coef)
    enc.close()
    ctx.free(coef)
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
        return statistics.median(got)
    ways, moved, scalers, dsts = {"crop": lambda: dec.get_frame_dev(planar)}, {"crop": n_streams * (fb + int(lib.pfv_padded_frame_bytes(w, h)))}, [], {}
    for sw, sh, dw, dh in scale_cases(w, h):
        sfb, dfb = int(lib.pfv_frame_bytes(sw, sh)), int(lib.pfv_frame_bytes(dw, dh))
        if (dw, dh) not in dsts:
            dsts[(dw, dh)] = ctx.alloc(dfb * n_streams) if (dw, dh) != (w, h) else planar
        for kind in ("bilinear", "bicubic", "lanczos3"):
            sc = pkg.Scaler(ctx, sw, sh, dw, dh, kind)
            scalers.append(sc)
            key = f"{sw}x{sh}->{dw}x{dh} {kind}"
            ways[key] = (lambda sc=sc, dst=dsts[(dw, dh)]: sc.run_dev(n_streams, f0, dst))      # the first sw x sh bytes of f0's frames serve as the smaller source too
            moved[key] = n_streams * (sfb + dfb)
    res = {k: [] for k in ways}
    for _ in range(rounds):
        for key, fn in ways.items():
            res[key].append(median_ms(fn))
    ctx.sync()
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    for sc in scalers:
        sc.close()
    dec.close()
    for p in [f0, planar] + [d for d in dsts.values() if d != planar]:
        ctx.free(p)
    over = lambda x, y: x / y if y else None      # noqa: E731  (an emulated device has no clock: its events are 0 ms apart)
    med = {k: statistics.median(v) for k, v in res.items()}
    gbps = {k: over(moved[k], med[k] * 1e6) for k in ways}
    rows = []
    for key in ways:
        rows.append({"shape": f"{n_streams} x {w}x{h}", "case": key, "ms": med[key], "bytes": moved[key], "GBps": gbps[key],
                     "rate_over_crop_rate": over(gbps[key], gbps["crop"]) if gbps[key] else None, "rounds_ms": res[key], "samples_per_round": samples})
    return rows


def time_ingest(pkg, ctx, fmt, chroma, n_streams=96, w=1920, h=1080, warmup=5, samples=30, rounds=3):
    lib = ctx._lib
    P = ctypes.c_void_p
    fb = int(lib.pfv_frame_bytes(w, h))
    m, c = pkg.quality.pix_format(fmt), pkg.quality.chroma_mode(chroma)
    bpp = int(lib.pfv_rgb_row_bytes(w, m)) // w
    f0, planar = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    rgb, rgb3 = ctx.alloc(w * h * bpp * n_streams), ctx.alloc(w * h * 3 * n_streams)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, f0)
    ctx.check(lib.pfv_frames_to_rgb_dev(ctx.handle, w, h, n_streams, P(f0), 0, 0, P(rgb), m, 0, 0))     # the pictures to ingest, in `fmt` and in RGB8
    ctx.check(lib.pfv_frames_to_rgb_dev(ctx.handle, w, h, n_streams, P(f0), 0, 0, P(rgb3), 0, 0, 0))
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

    def without():                                # one launch per stream: RGB8 in, POINT out, whatever `fmt` and `chroma` are
        for k in range(n_streams):
            ctx.check(lib.pfv_rgb_to_yuv420_dev(ctx.handle, P(rgb3 + k * w * h * 3), w, h, P(planar + k * fb)))
    ways = {"a_ingest": lambda: ctx.check(lib.pfv_frames_from_rgb_dev(ctx.handle, w, h, n_streams, P(rgb), m, 0, 0, P(planar), 0, c)),
            "b_per_stream": without,
            "c_present": lambda: ctx.check(lib.pfv_frames_to_rgb_dev(ctx.handle, w, h, n_streams, P(f0), 0, 0, P(rgb), m, 0, 0))}
    res = {k: [] for k in ways}
    for _ in range(rounds):                       # alternate, so that whatever else the box is doing meets all of them
        for key, fn in ways.items():
            res[key].append(median_ms(fn))
    ctx.sync()
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    for p in (f0, planar, rgb, rgb3):
        ctx.free(p)
    med = {k: statistics.median(v for v, _, _ in r) for k, r in res.items()}
    moved = {"a_ingest": n_streams * (w * h * bpp + fb), "b_per_stream": n_streams * (w * h * 3 + fb), "c_present": n_streams * (fb + w * h * bpp)}
    over = lambda x, y: x / y if y else None      # noqa: E731  (an emulated device has no clock: its events are 0 ms apart)
    gbps = {k: over(moved[k], med[k] * 1e6) for k in ways}
    return {"shape": f"{n_streams} x {w}x{h}", "format": fmt, "chroma": chroma, "samples_per_round": samples, "rounds": rounds,
            "a_ingest_ms": med["a_ingest"], "b_per_stream_ms": med["b_per_stream"], "c_present_ms": med["c_present"],
            "bytes": moved, "GBps": gbps, "a_over_b_time": over(med["a_ingest"], med["b_per_stream"]),
            "a_rate_over_c_rate": over(gbps["a_ingest"], gbps["c_present"]) if gbps["a_ingest"] else None, "rounds_ms": res}


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


def probe_sizes_line(pkg, ctx, w, h, kind, ladder):
    """probed against written payload bytes of the clip's first frame at every rung"""
    fr = pkg.VideoFrame.from_packed(w, h, pkg.SyntheticStream(w, h, kind=kind).frame(0))
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, frame_report=True, qualities=ladder)
    probed = [int(v) for v in enc.probe_iframe(fr)]
    written = []
    for r in range(len(ladder)):
        enc.set_rung(r)
        enc.encode_iframe(fr)
        written.append(enc.last_report.packet_bytes - 5)
    enc.close()
    return {"ladder": ladder, "width": w, "height": h, "kind": kind, "probed_bytes": probed, "written_bytes": written, "equal": probed == written}


def time_probe(pkg, ctx, n_streams, ladder, w=1920, h=1080, warmup=3, samples=20, rounds=3):
    lib = ctx._lib
    fb, tb, R = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h)), len(ladder)
    frames, coef, sizes = ctx.alloc(fb * n_streams), ctx.alloc(n_streams * tb * 512), ctx.alloc(n_streams * R * 4)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, frames)
    probe = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    upto = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full.enable_entropy()
    upto.enable_entropy(payload_cap=24)            # every payload is "over capacity": k_ent_init / k_ent_pack return at once
    e0, e1 = ctx.event(), ctx.event()

    def trial(enc):
        for r in range(R):
            enc.set_rung(r)
            enc.encode_iframe_dev(frames, coef)
            enc.pack_iframe_dev(coef)

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
        return statistics.median(got)
    res = {"probe": [], "trials_full": [], "trials_to_size": []}
    for _ in range(rounds):
        res["probe"].append(median_ms(lambda: probe.probe_iframe_dev(frames, sizes)))
        res["trials_to_size"].append(median_ms(lambda: trial(upto)))
        res["trials_full"].append(median_ms(lambda: trial(full)))
    # the answers: the probe's sizes against the trial encodes' (rung by rung, all streams)
    got = np.zeros((n_streams, R), np.uint32)
    ctx.download(got, sizes)
    same = True
    for r in range(R):
        full.set_rung(r)
        full.encode_iframe_dev(frames, coef)
        full.pack_iframe_dev(coef)
        same = same and bool(np.array_equal(full.payload_sizes(), got[:, r]))
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    for s in (probe, full, upto):
        s.close()
    for p in (frames, coef, sizes):
        ctx.free(p)
    a, b, bf = (statistics.median(res[k]) for k in ("probe", "trials_to_size", "trials_full"))
    spread = max(res["trials_to_size"]) - min(res["trials_to_size"])
    return {"shape": f"{n_streams} x {w}x{h}", "ladder": ladder, "samples_per_round": samples, "rounds": rounds,
            "probe_ms": a, "trials_to_size_ms": b, "trials_full_ms": bf, "trials_to_size_spread_ms": spread,
            "probe_over_trials_to_size": a / b if b else None, "probe_below_trials_by_more_than_spread": bool(a < b - spread),
            "rounds_ms": res, "sizes_equal_trial_encodes": same, "bytes_stream0": [int(v) for v in got[0]]}


def probe_rd_line(pkg, ctx, w, h, kind, ladder):
    """probed against written payload bytes and probed against reported squared error of the clip's first frame at every rung"""
    fr = pkg.VideoFrame.from_packed(w, h, pkg.SyntheticStream(w, h, kind=kind).frame(0))
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, frame_report=True, qualities=ladder)
    sizes, sse = enc.probe_iframe_rd(fr)
    probed, probed_sse = [int(v) for v in sizes], [[int(v) for v in row] for row in sse]
    written, reported, psnr = [], [], []
    for r in range(len(ladder)):
        enc.set_rung(r)
        enc.encode_iframe(fr)
        rep = enc.last_report
        written.append(rep.packet_bytes - 5)
        reported.append([int(v) for v in rep.sse])
        psnr.append(rep.psnr_yuv)
    enc.close()
    return {"ladder": ladder, "width": w, "height": h, "kind": kind, "probed_bytes": probed, "written_bytes": written, "probed_sse": probed_sse,
            "reported_sse": reported, "psnr_yuv": psnr, "equal": probed == written and probed_sse == reported}


def time_probe_rd(pkg, ctx, n_streams, ladder, w=1920, h=1080, warmup=3, samples=20, rounds=3):
    lib = ctx._lib
    fb, tb, R = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h)), len(ladder)
    frames, coef = ctx.alloc(fb * n_streams), ctx.alloc(n_streams * tb * 512)
    sizes, sse, sse_b = ctx.alloc(n_streams * R * 4), ctx.alloc(n_streams * R * 24), ctx.alloc(n_streams * 24)
    ctx.synth_frames_dev(w, h, np.arange(1, n_streams + 1, dtype=np.uint64), 0, frames)
    probe = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    upto = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    upto.enable_entropy(payload_cap=24)            # the stage "up to the size", as time_probe
    e0, e1 = ctx.event(), ctx.event()

    def trial():
        for r in range(R):
            upto.set_rung(r)
            upto.encode_iframe_dev(frames, coef)
            upto.pack_iframe_dev(coef)
            upto.distortion_dev(frames, sse_b)

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
        return statistics.median(got)
    res = {"rd_probe": [], "trials": [], "size_probe": []}
    for _ in range(rounds):
        res["rd_probe"].append(median_ms(lambda: probe.probe_iframe_rd_dev(frames, sizes, sse)))
        res["trials"].append(median_ms(trial))
        res["size_probe"].append(median_ms(lambda: probe.probe_iframe_dev(frames, sizes)))
    # the answers: the probe's against the trial encodes' (rung by rung, all streams)
    probe.probe_iframe_rd_dev(frames, sizes, sse)
    got, got_sse = np.zeros((n_streams, R), np.uint32), np.zeros((n_streams, R, 3), np.uint64)
    ctx.download(got, sizes)
    ctx.download(got_sse, sse)
    full = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full.enable_entropy()
    same_sizes, same_sse = [], []
    one = np.zeros((n_streams, 3), np.uint64)
    for r in range(R):
        full.set_rung(r)
        full.encode_iframe_dev(frames, coef)
        full.pack_iframe_dev(coef)
        full.distortion_dev(frames, sse_b)
        same_sizes.append(bool(np.array_equal(full.payload_sizes(), got[:, r])))
        ctx.download(one, sse_b)
        same_sse.append(bool(np.array_equal(one, got_sse[:, r])))
    ctx.event_destroy(e0); ctx.event_destroy(e1)
    for s in (probe, upto, full):
        s.close()
    for p in (frames, coef, sizes, sse, sse_b):
        ctx.free(p)
    a, b, c = (statistics.median(res[k]) for k in ("rd_probe", "trials", "size_probe"))
    spread = {k: max(v) - min(v) for k, v in res.items()}
    samples_n = n_streams * fb
    return {"shape": f"{n_streams} x {w}x{h}", "ladder": ladder, "samples_per_round": samples, "rounds": rounds,
            "A_rd_probe_ms": a, "B_trials_ms": b, "C_size_probe_ms": c, "spread_ms": spread, "A_over_B": a / b if b else None,
            "A_below_B_by_more_than_Bs_spread": bool(a < b - spread["trials"]), "distortion_half_ms": a - c, "rounds_ms": res,
            "sizes_equal_per_rung": same_sizes, "sse_equal_per_rung": same_sse, "bytes_stream0": [int(v) for v in got[0]],
            "psnr_yuv_all_streams": [pkg.psnr(int(got_sse[:, r].sum()), samples_n) for r in range(R)]}


def time_budget(pkg, ctx, ladder, w=1920, h=1080, n=12, rounds=3):
    """host milliseconds per encode_iframe of one pfv_encoder, i-frame budget off / on (a budget the middle rung meets)"""
    st = pkg.SyntheticStream(w, h)
    frs = [pkg.VideoFrame.from_packed(w, h, st.frame(t)) for t in range(n)]
    per = {False: [], True: []}
    chosen = set()
    for _ in range(rounds):
        for on in (False, True):
            enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=ladder)
            budget = int(enc.probe_iframe(frs[0])[len(ladder) // 2])
            enc.set_rung(len(ladder) // 2)
            if on:
                enc.set_iframe_budget(budget)
            secs = []
            for fr in frs:
                t0 = time.perf_counter()
                enc.encode_iframe(fr)
                secs.append(time.perf_counter() - t0)
                chosen.add((on, enc.rung))
            enc.close()
            per[on].append(statistics.median(secs[2:]) * 1e3)
    off, on_ms = statistics.median(per[False]), statistics.median(per[True])
    return {"shape": f"1 x {w}x{h}", "ladder": ladder, "iframe_ms_budget_off": off, "iframe_ms_budget_on": on_ms, "added_ms": on_ms - off,
            "rounds_ms": {"off": per[False], "on": per[True]}, "rungs_seen": sorted(chosen)}


def time_probe_p(pkg, ctx, n_streams, ladder, w=1920, h=1080, warmup=3, samples=20, rounds=3):
    lib = ctx._lib
    fb, tb, R = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h)), len(ladder)
    mid = R // 2
    f0, f1 = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    coef, mv, has = ctx.alloc(n_streams * tb * 512), ctx.alloc(n_streams * tb * 2), ctx.alloc(n_streams * tb)
    sizes = ctx.alloc(n_streams * R * 4)
    seeds = np.arange(1, n_streams + 1, dtype=np.uint64)
    ctx.synth_frames_dev(w, h, seeds, 0, f0)
    ctx.synth_frames_dev(w, h, seeds, 1, f1)
    probe = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    upto = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full.enable_entropy()
    upto.enable_entropy(payload_cap=24)            # every payload is "over capacity": k_ent_init / k_ent_pack return at once
    probe.set_rung(mid)
    probe.encode_iframe_dev(f0, coef)              # the state every measurement starts from: frame 0 as an i-frame at the middle rung
    ev = [(ctx.event(), ctx.event()) for _ in range(R)]

    def elapsed(pair):
        ms = ctypes.c_float()
        ctx.check(lib.pfv_event_elapsed_ms(pair[0], pair[1], ctypes.byref(ms)))
        return float(ms.value)

    def sample_probe():
        ctx.record(ev[0][0])
        probe.probe_pframe_dev(f1, sizes)
        ctx.record(ev[0][1])
        return elapsed(ev[0])

    def sample_trials(enc):
        for r in range(R):
            enc.set_rung(mid)
            enc.encode_iframe_dev(f0, coef)        # outside the pair: prev_frame back to the state the probe sees
            enc.set_rung(r)
            ctx.record(ev[r][0])
            enc.encode_pframe_dev(f1, mv, has, coef)
            enc.pack_pframe_dev(mv, has, coef)
            ctx.record(ev[r][1])
        return sum(elapsed(p) for p in ev)

    def median_ms(fn):
        got = [fn() for _ in range(warmup + samples)]
        return statistics.median(got[warmup:])
    res = {"probe": [], "trials_full": [], "trials_to_size": []}
    for _ in range(rounds):
        res["probe"].append(median_ms(sample_probe))
        res["trials_to_size"].append(median_ms(lambda: sample_trials(upto)))
        res["trials_full"].append(median_ms(lambda: sample_trials(full)))
    got = np.zeros((n_streams, R), np.uint32)
    ctx.download(got, sizes)
    same = True
    for r in range(R):
        full.set_rung(mid)
        full.encode_iframe_dev(f0, coef)
        full.set_rung(r)
        full.encode_pframe_dev(f1, mv, has, coef)
        full.pack_pframe_dev(mv, has, coef)
        same = same and bool(np.array_equal(full.payload_sizes(), got[:, r]))
    for a, b in ev:
        ctx.event_destroy(a); ctx.event_destroy(b)
    for s_ in (probe, full, upto):
        s_.close()
    for p in (f0, f1, coef, mv, has, sizes):
        ctx.free(p)
    a, b, bf = (statistics.median(res[k]) for k in ("probe", "trials_to_size", "trials_full"))
    spread = max(res["trials_to_size"]) - min(res["trials_to_size"])
    return {"shape": f"{n_streams} x {w}x{h}", "ladder": ladder, "samples_per_round": samples, "rounds": rounds,
            "probe_ms": a, "trials_to_size_ms": b, "trials_full_ms": bf, "trials_to_size_spread_ms": spread,
            "probe_over_trials_to_size": a / b if b else None, "probe_below_trials_by_more_than_spread": bool(a < b - spread),
            "rounds_ms": res, "sizes_equal_trial_encodes": same, "bytes_stream0": [int(v) for v in got[0]]}


def time_pframe_modes(pkg, ctx, ladder, w=1920, h=1080, n=14, rounds=3):
    """host milliseconds per frame of one pfv_encoder behind an i-frame: encode_pframe with the soft budget, encode_pframe with the hard budget
    (the probe on), encode_frame (automatic type, no budget)"""
    st = pkg.SyntheticStream(w, h)
    frs = [pkg.VideoFrame.from_packed(w, h, st.frame(t)) for t in range(n)]
    per = {"pframe_soft": [], "pframe_hard": [], "encode_frame": []}
    seen = {k: set() for k in per}
    for _ in range(rounds):
        for mode in per:
            enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=ladder)
            enc.set_rung(len(ladder) // 2)
            enc.encode_iframe(frs[0])
            budget = int(enc.probe_pframe(frs[1])[len(ladder) // 2])
            if mode != "encode_frame":
                enc.set_rate(budget)
                enc.set_pframe_probe(mode == "pframe_hard")
            secs = []
            for fr in frs[1:]:
                t0 = time.perf_counter()
                kind = enc.encode_frame(fr) if mode == "encode_frame" else (enc.encode_pframe(fr), 2)[1]
                secs.append(time.perf_counter() - t0)
                seen[mode].add((kind, enc.rung))
            enc.close()
            per[mode].append(statistics.median(secs[1:]) * 1e3)
    out = {"shape": f"1 x {w}x{h}", "ladder": ladder, "rounds_ms": per, "types_and_rungs_seen": {k: sorted(v) for k, v in seen.items()}}
    for k, v in per.items():
        out[k + "_ms"] = statistics.median(v)
    return out


def pprobe_sizes_line(pkg, ctx, w, h, kind, ladder):
    """probed against written payload bytes of the clip's second frame as a p-frame behind its first at every rung"""
    st = pkg.SyntheticStream(w, h, kind=kind)
    f0, f1 = (pkg.VideoFrame.from_packed(w, h, st.frame(t)) for t in (0, 1))
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, frame_report=True, qualities=ladder)
    probed, written = None, []
    for r in range(len(ladder)):
        enc.set_rung(len(ladder) // 2)
        enc.encode_iframe(f0)
        probed = [int(v) for v in enc.probe_pframe(f1)]
        enc.set_rung(r)
        enc.encode_pframe(f1)
        written.append(enc.last_report.packet_bytes - 5)
    enc.close()
    return {"ladder": ladder, "width": w, "height": h, "kind": kind, "probed_bytes": probed, "written_bytes": written, "equal": probed == written}


def pprobe_rd_line(pkg, ctx, w, h, kind, ladder):
    """probed against written payload bytes and reported squared error of the clip's second frame as a p-frame behind its first at every rung"""
    st = pkg.SyntheticStream(w, h, kind=kind)
    f0, f1 = (pkg.VideoFrame.from_packed(w, h, st.frame(t)) for t in (0, 1))
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, frame_report=True, qualities=ladder)
    probed, probed_sse, written, reported, psnr = None, None, [], [], []
    for r in range(len(ladder)):
        enc.set_rung(len(ladder) // 2)
        enc.encode_iframe(f0)
        sizes, sse = enc.probe_pframe_rd(f1)
        probed, probed_sse = [int(v) for v in sizes], [[int(v) for v in row] for row in sse]
        enc.set_rung(r)
        enc.encode_pframe(f1)
        rep = enc.last_report
        written.append(rep.packet_bytes - 5)
        reported.append([int(v) for v in rep.sse])
        psnr.append(rep.psnr_yuv)
    enc.close()
    return {"ladder": ladder, "width": w, "height": h, "kind": kind, "probed_bytes": probed, "written_bytes": written, "probed_sse": probed_sse,
            "reported_sse": reported, "psnr_yuv": psnr, "equal": probed == written and probed_sse == reported}


def time_probe_p_rd(pkg, ctx, n_streams, ladder, w=1920, h=1080, warmup=3, samples=20, rounds=3):
    lib = ctx._lib
    fb, tb, R = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h)), len(ladder)
    mid = R // 2
    f0, f1 = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    coef, mv, has = ctx.alloc(n_streams * tb * 512), ctx.alloc(n_streams * tb * 2), ctx.alloc(n_streams * tb)
    sizes, sse, sse_b = ctx.alloc(n_streams * R * 4), ctx.alloc(n_streams * R * 24), ctx.alloc(n_streams * 24)
    seeds = np.arange(1, n_streams + 1, dtype=np.uint64)
    ctx.synth_frames_dev(w, h, seeds, 0, f0)
    ctx.synth_frames_dev(w, h, seeds, 1, f1)
    probe = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    upto = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full.enable_entropy()
    upto.enable_entropy(payload_cap=24)            # the stage "up to the size", as time_probe_p
    probe.set_rung(mid)
    probe.encode_iframe_dev(f0, coef)              # the state every measurement starts from: frame 0 as an i-frame at the middle rung
    ev = [(ctx.event(), ctx.event()) for _ in range(R)]

    def elapsed(pair):
        ms = ctypes.c_float()
        ctx.check(lib.pfv_event_elapsed_ms(pair[0], pair[1], ctypes.byref(ms)))
        return float(ms.value)

    def sample(fn):
        ctx.record(ev[0][0])
        fn()
        ctx.record(ev[0][1])
        return elapsed(ev[0])

    def sample_trials():
        for r in range(R):
            upto.set_rung(mid)
            upto.encode_iframe_dev(f0, coef)       # outside the pair: prev_frame back to the state the probe sees
            ctx.record(ev[r][0])
            upto.set_rung(r)
            upto.encode_pframe_dev(f1, mv, has, coef)
            upto.pack_pframe_dev(mv, has, coef)
            upto.distortion_dev(f1, sse_b)
            ctx.record(ev[r][1])
        return sum(elapsed(p) for p in ev)

    def median_ms(fn):
        got = [fn() for _ in range(warmup + samples)]
        return statistics.median(got[warmup:])
    res = {"rd_probe": [], "trials": [], "size_probe": []}
    for _ in range(rounds):
        res["rd_probe"].append(median_ms(lambda: sample(lambda: probe.probe_pframe_rd_dev(f1, sizes, sse))))
        res["trials"].append(median_ms(sample_trials))
        res["size_probe"].append(median_ms(lambda: sample(lambda: probe.probe_pframe_dev(f1, sizes))))
    # the answers: the probe's against the trial encodes' (rung by rung, all streams)
    probe.probe_pframe_rd_dev(f1, sizes, sse)
    got, got_sse = np.zeros((n_streams, R), np.uint32), np.zeros((n_streams, R, 3), np.uint64)
    ctx.download(got, sizes)
    ctx.download(got_sse, sse)
    same_sizes, same_sse = [], []
    one = np.zeros((n_streams, 3), np.uint64)
    for r in range(R):
        full.set_rung(mid)
        full.encode_iframe_dev(f0, coef)
        full.set_rung(r)
        full.encode_pframe_dev(f1, mv, has, coef)
        full.pack_pframe_dev(mv, has, coef)
        full.distortion_dev(f1, sse_b)
        same_sizes.append(bool(np.array_equal(full.payload_sizes(), got[:, r])))
        ctx.download(one, sse_b)
        same_sse.append(bool(np.array_equal(one, got_sse[:, r])))
    for a, b in ev:
        ctx.event_destroy(a); ctx.event_destroy(b)
    for s_ in (probe, full, upto):
        s_.close()
    for p in (f0, f1, coef, mv, has, sizes, sse, sse_b):
        ctx.free(p)
    a, b, c = (statistics.median(res[k]) for k in ("rd_probe", "trials", "size_probe"))
    spread = {k: max(v) - min(v) for k, v in res.items()}
    samples_n = n_streams * fb
    return {"shape": f"{n_streams} x {w}x{h}", "ladder": ladder, "samples_per_round": samples, "rounds": rounds,
            "A_rd_probe_ms": a, "B_trials_ms": b, "C_size_probe_ms": c, "spread_ms": spread, "A_over_B": a / b if b else None,
            "A_below_B_by_more_than_Bs_spread": bool(a < b - spread["trials"]), "distortion_half_ms": a - c,
            "distortion_half_ms_per_rung": (a - c) / R, "rounds_ms": res,
            "sizes_equal_per_rung": same_sizes, "sse_equal_per_rung": same_sse, "bytes_stream0": [int(v) for v in got[0]],
            "psnr_yuv_all_streams": [pkg.psnr(int(got_sse[:, r].sum()), samples_n) for r in range(R)]}


def time_pframe_floor_modes(pkg, ctx, ladder, w=1920, h=1080, n=14, rounds=3):
    """host milliseconds per frame of one pfv_encoder behind an i-frame: encode_pframe and encode_frame, p-frame quality floor off / on (a
    floor the middle rung of frame 1 meets)"""
    st = pkg.SyntheticStream(w, h)
    frs = [pkg.VideoFrame.from_packed(w, h, st.frame(t)) for t in range(n)]
    per = {"pframe": [], "pframe_floor": [], "encode_frame": [], "encode_frame_floor": []}
    seen = {k: set() for k in per}
    for _ in range(rounds):
        for mode in per:
            enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, qualities=ladder)
            enc.set_rung(len(ladder) // 2)
            enc.encode_iframe(frs[0])
            if mode.endswith("_floor"):
                sse = enc.probe_pframe_rd(frs[1])[1]
                enc.set_pframe_quality_floor(pkg.psnr(int(sse[len(ladder) // 2].sum()), int(ctx._lib.pfv_frame_bytes(w, h))))
            secs = []
            for fr in frs[1:]:
                t0 = time.perf_counter()
                kind = enc.encode_frame(fr) if mode.startswith("encode_frame") else (enc.encode_pframe(fr), 2)[1]
                secs.append(time.perf_counter() - t0)
                seen[mode].add((kind, enc.rung))
            enc.close()
            per[mode].append(statistics.median(secs[1:]) * 1e3)
    out = {"shape": f"1 x {w}x{h}", "ladder": ladder, "rounds_ms": per, "types_and_rungs_seen": {k: sorted(v) for k, v in seen.items()}}
    for k, v in per.items():
        out[k + "_ms"] = statistics.median(v)
    return out


def probe_ssim_line(pkg, ctx, w, h, kind, ladder, pframe):
    """probed against written payload bytes, reported squared error and reported SSIM sums at every rung: the clip's first frame as an i-frame,
    or its second frame as a p-frame behind the first at the middle rung"""
    st = pkg.SyntheticStream(w, h, kind=kind)
    f0, f1 = (pkg.VideoFrame.from_packed(w, h, st.frame(t)) for t in (0, 1))
    enc = pkg.Encoder(io.BytesIO(), w, h, 30, None, ctx, frame_report=True, frame_ssim=True, qualities=ladder)
    probed, written, ssim = None, [], []
    for r in range(len(ladder)):
        if pframe:
            enc.set_rung(len(ladder) // 2)
            enc.encode_iframe(f0)
        got = enc.probe_pframe_ssim(f1) if pframe else enc.probe_iframe_ssim(f0)
        got = [[int(v) for v in np.asarray(x).reshape(-1)] for x in got]
        assert probed is None or probed == got
        probed = got
        enc.set_rung(r)
        enc.encode_pframe(f1) if pframe else enc.encode_iframe(f0)
        rep, ss = enc.last_report, enc.last_ssim
        written.append((rep.packet_bytes - 5, [int(v) for v in rep.sse], [int(v) for v in ss.q24]))
        ssim.append(ss.ssim_all)
    enc.close()
    flat = [[x[0] for x in written], [v for x in written for v in x[1]], [v for x in written for v in x[2]]]
    return {"ladder": ladder, "width": w, "height": h, "kind": kind, "pframe": pframe, "probed_bytes": probed[0], "probed_q24": probed[2],
            "ssim_all": ssim, "equal": probed == flat}


def time_probe_ssim(pkg, ctx, n_streams, ladder, pframe, w=1920, h=1080, warmup=3, samples=20, rounds=3):
    """A = the SSIM probe's launch group; B = what it replaces on the same build, per rung a trial encode up to the size,
    pfv_enc_distortion_dev and pfv_enc_ssim_dev; C = the RD probe.  Device events, warmed shapes; the answers compared rung by rung."""
    lib = ctx._lib
    fb, tb, R = int(lib.pfv_frame_bytes(w, h)), int(lib.pfv_total_blocks(w, h)), len(ladder)
    mid = R // 2
    f0, f1 = ctx.alloc(fb * n_streams), ctx.alloc(fb * n_streams)
    coef, mv, has = ctx.alloc(n_streams * tb * 512), ctx.alloc(n_streams * tb * 2), ctx.alloc(n_streams * tb)
    sizes, sse, q24 = ctx.alloc(n_streams * R * 4), ctx.alloc(n_streams * R * 24), ctx.alloc(n_streams * R * 24)
    sse_b, q_b = ctx.alloc(n_streams * 24), ctx.alloc(n_streams * 24)
    seeds = np.arange(1, n_streams + 1, dtype=np.uint64)
    ctx.synth_frames_dev(w, h, seeds, 0, f0)
    ctx.synth_frames_dev(w, h, seeds, 1, f1)
    probe = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    upto = pkg.EncoderSession(ctx, w, h, None, n_streams, qualities=ladder)
    full.enable_entropy()
    upto.enable_entropy(payload_cap=24)            # the stage "up to the size", as time_probe
    probe.set_rung(mid)
    probe.encode_iframe_dev(f0, coef)              # p-frames: frame 0 as an i-frame at the middle rung is the state every measurement starts from
    frame = f1 if pframe else f0
    ev = [(ctx.event(), ctx.event()) for _ in range(R)]

    def elapsed(pair):
        ms = ctypes.c_float()
        ctx.check(lib.pfv_event_elapsed_ms(pair[0], pair[1], ctypes.byref(ms)))
        return float(ms.value)

    def sample(fn):
        ctx.record(ev[0][0])
        fn()
        ctx.record(ev[0][1])
        return elapsed(ev[0])

    def trial_rung(s, r):
        if pframe:
            s.set_rung(mid)
            s.encode_iframe_dev(f0, coef)          # outside the pair: prev_frame back to the state the probe sees
        ctx.record(ev[r][0])
        s.set_rung(r)
        if pframe:
            s.encode_pframe_dev(f1, mv, has, coef)
            s.pack_pframe_dev(mv, has, coef)
        else:
            s.encode_iframe_dev(f0, coef)
            s.pack_iframe_dev(coef)
        s.distortion_dev(frame, sse_b)
        s.ssim_dev(frame, q_b)
        ctx.record(ev[r][1])

    def sample_trials():
        for r in range(R):
            trial_rung(upto, r)
        return sum(elapsed(p) for p in ev)

    def median_ms(fn):
        got = [fn() for _ in range(warmup + samples)]
        return statistics.median(got[warmup:])
    ssim_probe = (lambda: probe.probe_pframe_ssim_dev(f1, sizes, sse, q24)) if pframe else (lambda: probe.probe_iframe_ssim_dev(f0, sizes, sse, q24))
    rd_probe = (lambda: probe.probe_pframe_rd_dev(f1, sizes, sse)) if pframe else (lambda: probe.probe_iframe_rd_dev(f0, sizes, sse))
    res = {"ssim_probe": [], "trials": [], "rd_probe": []}
    for _ in range(rounds):
        res["ssim_probe"].append(median_ms(lambda: sample(ssim_probe)))
        res["trials"].append(median_ms(sample_trials))
        res["rd_probe"].append(median_ms(lambda: sample(rd_probe)))
    ssim_probe()
    got, got_sse, got_q = np.zeros((n_streams, R), np.uint32), np.zeros((n_streams, R, 3), np.uint64), np.zeros((n_streams, R, 3), np.int64)
    ctx.download(got, sizes)
    ctx.download(got_sse, sse)
    ctx.download(got_q, q24)
    same = {"sizes": [], "sse": [], "q24": []}
    one, one_q = np.zeros((n_streams, 3), np.uint64), np.zeros((n_streams, 3), np.int64)
    for r in range(R):
        trial_rung(full, r)
        same["sizes"].append(bool(np.array_equal(full.payload_sizes(), got[:, r])))
        ctx.download(one, sse_b)
        ctx.download(one_q, q_b)
        same["sse"].append(bool(np.array_equal(one, got_sse[:, r])))
        same["q24"].append(bool(np.array_equal(one_q, got_q[:, r])))
    for a, b in ev:
        ctx.event_destroy(a); ctx.event_destroy(b)
    for s_ in (probe, full, upto):
        s_.close()
    for p in (f0, f1, coef, mv, has, sizes, sse, q24, sse_b, q_b):
        ctx.free(p)
    a, b, c = (statistics.median(res[k]) for k in ("ssim_probe", "trials", "rd_probe"))
    spread = {k: max(v) - min(v) for k, v in res.items()}
    windows = sum(pkg.ssim_windows(w, h)) if hasattr(pkg, "ssim_windows") else None
    return {"shape": f"{n_streams} x {w}x{h}", "pframe": pframe, "ladder": ladder, "samples_per_round": samples, "rounds": rounds,
            "A_ssim_probe_ms": a, "B_trials_ms": b, "C_rd_probe_ms": c, "spread_ms": spread, "A_over_B": a / b if b else None,
            "A_below_B_by_more_than_Bs_spread": bool(a < b - spread["trials"]), "ssim_half_ms": a - c, "rounds_ms": res,
            "map_bytes": n_streams * tb * (R * 128 + 64), "equal_per_rung": same, "bytes_stream0": [int(v) for v in got[0]],
            "ssim_all_streams": [float(got_q[:, r].sum()) / (16777216.0 * windows * n_streams) for r in range(R)] if windows else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("frames", type=int)
    ap.add_argument("--gop", type=int, default=15)
    ap.add_argument("--kind", choices=("pan", "low_motion", "static"), default="pan")
    ap.add_argument("--qualities", default="0,2,5,10")
    ap.add_argument("--time-kernel", action="store_true")
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--probe-p", action="store_true")
    ap.add_argument("--probe-rd", action="store_true")
    ap.add_argument("--probe-p-rd", action="store_true")
    ap.add_argument("--probe-ssim", action="store_true")
    ap.add_argument("--probe-p-ssim", action="store_true")
    ap.add_argument("--ssim", action="store_true")
    ap.add_argument("--time-ssim", action="store_true")
    ap.add_argument("--deblock", action="store_true")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--time-deblock", action="store_true")
    ap.add_argument("--time-present", action="store_true")
    ap.add_argument("--time-ingest", action="store_true")
    ap.add_argument("--time-scale", action="store_true")
    ap.add_argument("--denoise", default=None, metavar="SS,ST")
    ap.add_argument("--time-denoise", action="store_true")
    ap.add_argument("--search", default=None, metavar="full[,R]|hier,R")
    ap.add_argument("--pan", default=None, metavar="DX,DY")
    ap.add_argument("--time-search", action="store_true")
    ap.add_argument("--scene-cut", nargs="?", const="176,5", default=None, metavar="THRESHOLD,R")
    ap.add_argument("--time-scene", action="store_true")
    a = ap.parse_args()
    assert a.frames >= 1 and a.gop >= 1
    pkg = load()
    with pkg.Context(0) as ctx:
        for q in [int(x) for x in a.qualities.split(",") if x != ""]:
            line = rd_line(pkg, ctx, a.width, a.height, a.frames, a.gop, a.kind, q, with_ssim=a.ssim)
            if a.deblock:
                line.update(deblock_line(pkg, ctx, a.width, a.height, a.frames, a.gop, a.kind, q, dump=a.dump))
            if a.denoise:
                ss, st = (int(x) for x in a.denoise.split(","))
                line.update(denoise_line(pkg, ctx, a.width, a.height, a.frames, a.gop, a.kind, q, ss, st, dump=a.dump))
            if a.search:
                parts = a.search.split(",")
                assert (parts[0] == "full" and len(parts) <= 2) or (parts[0] == "hier" and len(parts) == 2), "--search full[,R] or hier,R"
                pan = tuple(int(x) for x in a.pan.split(",")) if a.pan else None
                line.update(search_line(pkg, ctx, a.width, a.height, a.frames, a.gop, a.kind, q, int(parts[1]) if len(parts) == 2 else 15, mode=parts[0], pan=pan))
            print(json.dumps(line), flush=True)
        if a.time_search:
            emu = bool(os.environ.get("PFV_HIP_LIB"))      # another build of the C ABI (the CPU emulator): nothing to time, the row only
            kw = dict(n_streams=2, w=a.width, h=a.height, warmup=1, samples=2, rounds=1) if emu else {}
            print(json.dumps({"time_search": time_search(pkg, ctx, **kw)}), flush=True)
        if a.scene_cut:
            thr, rad = (int(x) for x in a.scene_cut.split(","))
            for q in [int(x) for x in a.qualities.split(",") if x != ""]:
                print(json.dumps({"scene_cut": scene_cut_line(pkg, ctx, a.width, a.height, a.frames, q, thr, rad)}), flush=True)
        if a.time_scene:
            emu = bool(os.environ.get("PFV_HIP_LIB"))      # another build of the C ABI (the CPU emulator): nothing to time, the row only
            kw = dict(n_streams=2, w=a.width, h=a.height, clip=(a.width, a.height, 3), warmup=1, samples=2, rounds=1) if emu else {}
            print(json.dumps({"time_scene": time_scene(pkg, ctx, **kw)}), flush=True)
        if a.time_ssim:
            print(json.dumps({"time_ssim": time_ssim(pkg, ctx)}), flush=True)
        if a.time_deblock:
            print(json.dumps({"time_deblock": time_deblock(pkg, ctx)}), flush=True)
        if a.time_denoise:
            emu = bool(os.environ.get("PFV_HIP_LIB"))      # another build of the C ABI (the CPU emulator): nothing to time, the row only
            kw = dict(n_streams=1, w=a.width, h=a.height, warmup=1, samples=2, rounds=1) if emu else {}
            print(json.dumps({"time_denoise": time_denoise(pkg, ctx, **kw)}), flush=True)
        if a.time_present:
            emu = bool(os.environ.get("PFV_HIP_LIB"))      # another build of the C ABI (the CPU emulator): nothing to time, the rows only
            for shape in ([] if emu else [dict(n_streams=96, w=1920, h=1080)]) + [dict(n_streams=1, w=a.width, h=a.height)]:
                for fmt in ("rgb8", "rgba8", "bgra8"):
                    kw = dict(warmup=1, samples=2, rounds=1) if emu else {}
                    print(json.dumps({"time_present": time_present(pkg, ctx, fmt, **shape, **kw)}), flush=True)
        if a.time_ingest:
            emu = bool(os.environ.get("PFV_HIP_LIB"))      # another build of the C ABI (the CPU emulator): nothing to time, the rows only
            for shape in ([] if emu else [dict(n_streams=96, w=1920, h=1080)]) + [dict(n_streams=1, w=a.width, h=a.height)]:
                for fmt in ("rgb8", "rgba8", "bgra8"):
                    for chroma in ("point", "box"):
                        kw = dict(warmup=1, samples=2, rounds=1) if emu else {}
                        print(json.dumps({"time_ingest": time_ingest(pkg, ctx, fmt, chroma, **shape, **kw)}), flush=True)
        if a.time_scale:
            emu = bool(os.environ.get("PFV_HIP_LIB"))      # another build of the C ABI (the CPU emulator): nothing to time, the rows only
            for row in (time_scale(pkg, ctx, 1, a.width, a.height, warmup=1, samples=2, rounds=1) if emu else time_scale(pkg, ctx)):
                print(json.dumps({"time_scale": row}), flush=True)
        if a.time_kernel:
            print(json.dumps({"time_kernel": time_kernels(pkg, ctx)}), flush=True)
        if a.probe:
            ladder = [int(x) for x in a.qualities.split(",") if x != ""]
            print(json.dumps({"probe_sizes": probe_sizes_line(pkg, ctx, a.width, a.height, a.kind, ladder)}), flush=True)
            if os.environ.get("PFV_HIP_LIB"):          # another build of the C ABI (the CPU emulator): nothing to time
                return
            for n_streams in (96, 1):
                for lad in ([0, 2, 5, 7, 10], list(range(11))):
                    print(json.dumps({"probe_timing": time_probe(pkg, ctx, n_streams, lad)}), flush=True)
            print(json.dumps({"probe_budget_latency": time_budget(pkg, ctx, [0, 2, 5, 7, 10])}), flush=True)
        if a.probe_p:
            ladder = [int(x) for x in a.qualities.split(",") if x != ""]
            print(json.dumps({"pprobe_sizes": pprobe_sizes_line(pkg, ctx, a.width, a.height, a.kind, ladder)}), flush=True)
            if os.environ.get("PFV_HIP_LIB"):          # another build of the C ABI (the CPU emulator): nothing to time
                return
            for n_streams in (96, 1):
                for lad in ([0, 2, 5, 7, 10], list(range(11))):
                    print(json.dumps({"pprobe_timing": time_probe_p(pkg, ctx, n_streams, lad)}), flush=True)
            print(json.dumps({"pprobe_encoder_latency": time_pframe_modes(pkg, ctx, [0, 2, 5, 7, 10])}), flush=True)
        if a.probe_rd:
            ladder = [int(x) for x in a.qualities.split(",") if x != ""]
            print(json.dumps({"probe_rd": probe_rd_line(pkg, ctx, a.width, a.height, a.kind, ladder)}), flush=True)
            if os.environ.get("PFV_HIP_LIB"):          # another build of the C ABI (the CPU emulator): nothing to time
                return
            for lad in ([0, 2, 5, 7, 10], list(range(11))):
                print(json.dumps({"probe_rd_timing": time_probe_rd(pkg, ctx, 96, lad)}), flush=True)
        if a.probe_p_rd:
            ladder = [int(x) for x in a.qualities.split(",") if x != ""]
            print(json.dumps({"pprobe_rd": pprobe_rd_line(pkg, ctx, a.width, a.height, a.kind, ladder)}), flush=True)
            if os.environ.get("PFV_HIP_LIB"):          # another build of the C ABI (the CPU emulator): nothing to time
                return
            for lad in ([0, 2, 5, 7, 10], list(range(11))):
                print(json.dumps({"pprobe_rd_timing": time_probe_p_rd(pkg, ctx, 96, lad)}), flush=True)
            print(json.dumps({"pprobe_rd_encoder_latency": time_pframe_floor_modes(pkg, ctx, [0, 2, 5, 7, 10])}), flush=True)
        for on, pframe in ((a.probe_ssim, False), (a.probe_p_ssim, True)):
            if not on:
                continue
            ladder = [int(x) for x in a.qualities.split(",") if x != ""]
            print(json.dumps({"probe_ssim": probe_ssim_line(pkg, ctx, a.width, a.height, a.kind, ladder, pframe)}), flush=True)
            if os.environ.get("PFV_HIP_LIB"):          # another build of the C ABI (the CPU emulator): nothing to time
                continue
            for lad in ([0, 2, 5, 7, 10], list(range(11))):
                print(json.dumps({"probe_ssim_timing": time_probe_ssim(pkg, ctx, 96, lad, pframe)}), flush=True)


if __name__ == "__main__":
    main()
