"""Distortion measured on the device (include/pfv_hip_ext.h, "distortion on the device"): squared error per plane and per
macroblock between frames, PSNR, and the frame report of :class:`Encoder`; and structural similarity ("structural similarity on the
device"): the SSIM sums per plane and per macroblock in 2^-24 fixed point, the mean from them, and the frame SSIM of :class:`Encoder`; and the out-of-loop deblocking filter of the frames that are shown (k_deblock).
The sums come from the k_sse_* and k_ssim_* kernels (csrc/pfv_quality_kernels.hip, csrc/pfv_ssim_kernels.hip); this module only marshals.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .context import Context, ptr


def psnr(sse: int, n_samples: int) -> float:
    """10 log10(255^2 n / sse) in double; +inf for sse == 0, nan for n == 0 (pfv_psnr)"""
    return float(_lib.load().pfv_psnr(int(sse), int(n_samples)))


def frames_sse(ctx: Context, width: int, height: int, a, b, mb_map: bool = False):
    """squared error between packed Y|U|V frames `a` and `b` (uint8, n frames each): uint64 [n, 3] per plane, and with mb_map the
    per-macroblock map uint32 [n, total_blocks] as well (pfv_frames_sse)"""
    fb = int(ctx._lib.pfv_frame_bytes(int(width), int(height)))
    fa = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    fb_ = fa if b is a else np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    assert fb > 0 and fa.size == fb_.size and fa.size % fb == 0 and fa.size
    n = fa.size // fb
    sse = np.zeros((n, 3), dtype=np.uint64)
    mb = np.zeros((n, int(ctx._lib.pfv_total_blocks(int(width), int(height)))), dtype=np.uint32) if mb_map else None
    ctx.check(ctx._lib.pfv_frames_sse(ctx.handle, int(width), int(height), n, ptr(fa), ptr(fb_), ptr(sse), ptr(mb) if mb_map else None))
    return (sse, mb) if mb_map else sse


def ssim(q24_sum: int, windows: int) -> float:
    """q24_sum / (2^24 windows) in double: the mean SSIM of the windows; nan for windows == 0 (pfv_ssim)"""
    return float(_lib.load().pfv_ssim(int(q24_sum), int(windows)))


def ssim_windows(width: int, height: int) -> tuple:
    """SSIM windows per plane (Y, U, V) of a width x height frame (pfv_ssim_windows)"""
    out = (ctypes.c_uint32 * 3)()
    rc = _lib.load().pfv_ssim_windows(int(width), int(height), out)
    if rc != _lib.PFV_OK:
        raise _lib.PfvError(rc, "pfv_ssim_windows: width/height must be positive, even and fit u16")
    return tuple(int(v) for v in out)


def frames_ssim(ctx: Context, width: int, height: int, a, b, mb_map: bool = False):
    """SSIM sums between packed Y|U|V frames `a` and `b` (uint8, n frames each): int64 [n, 3] per plane in 2^-24 fixed point (divide with
    :func:`ssim` by :func:`ssim_windows`), and with mb_map the per-macroblock map int32 [n, total_blocks] as well (pfv_frames_ssim)"""
    fb = int(ctx._lib.pfv_frame_bytes(int(width), int(height)))
    fa = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    fb_ = fa if b is a else np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    assert fb > 0 and fa.size == fb_.size and fa.size % fb == 0 and fa.size
    n = fa.size // fb
    sums = np.zeros((n, 3), dtype=np.int64)
    mb = np.zeros((n, int(ctx._lib.pfv_total_blocks(int(width), int(height)))), dtype=np.int32) if mb_map else None
    ctx.check(ctx._lib.pfv_frames_ssim(ctx.handle, int(width), int(height), n, ptr(fa), ptr(fb_), ptr(sums), ptr(mb) if mb_map else None))
    return (sums, mb) if mb_map else sums


DEBLOCK_MODES = {"off": _lib.PFV_DEBLOCK_OFF, "auto": _lib.PFV_DEBLOCK_AUTO, "fixed": _lib.PFV_DEBLOCK_FIXED}


def deblock_args(mode, strength):
    """(mode, strength pointer) of pfv_dec_set_deblock / pfv_decoder_set_deblock: mode "off" / "auto" / "fixed" or a PFV_DEBLOCK_* value;
    giving strengths alone means "fixed".  The array is returned as well: it must outlive the call."""
    if mode is None:
        mode = "fixed" if strength is not None else "auto"
    m = DEBLOCK_MODES[mode] if isinstance(mode, str) else int(mode)
    st = None if strength is None else np.ascontiguousarray(strength, dtype=np.uint8).reshape(3)
    return m, (ptr(st) if st is not None else None), st


def deblock_strength(qtable) -> int:
    """the automatic deblocking strength of a q-table, min(12, q[0] >> 1) (pfv_deblock_strength)"""
    q = np.ascontiguousarray(qtable, dtype=np.int32).reshape(64)
    return int(_lib.load().pfv_deblock_strength(ptr(q)))


def frames_deblock(ctx: Context, width: int, height: int, frames, strength) -> np.ndarray:
    """the out-of-loop deblocking filter (include/pfv_hip_ext.h, "out-of-loop deblocking") on packed Y|U|V frames (uint8, n frames) at the
    strengths (Y, U, V), each 0..12: uint8 [n, frame_bytes] (pfv_frames_deblock)"""
    fb = int(ctx._lib.pfv_frame_bytes(int(width), int(height)))
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    assert fb > 0 and f.size % fb == 0 and f.size
    n = f.size // fb
    st = np.ascontiguousarray(strength, dtype=np.uint8).reshape(3)
    out = np.empty((n, fb), dtype=np.uint8)
    ctx.check(ctx._lib.pfv_frames_deblock(ctx.handle, int(width), int(height), n, ptr(f), ptr(out), ptr(st)))
    return out


PIX_FORMATS = {"rgb8": _lib.PFV_PIX_RGB8, "rgba8": _lib.PFV_PIX_RGBA8, "bgra8": _lib.PFV_PIX_BGRA8}


def pix_format(fmt) -> int:
    """a pixel format of the RGB outputs: "rgb8" / "rgba8" / "bgra8" or a PFV_PIX_* value"""
    return PIX_FORMATS[fmt.lower()] if isinstance(fmt, str) else int(fmt)


def rgb_shape(ctx: Context, width: int, height: int, fmt: int) -> tuple:
    """(height, width, bytes per pixel) of one tight picture (pfv_rgb_row_bytes); raises for a format that does not exist"""
    row = int(ctx._lib.pfv_rgb_row_bytes(int(width), int(fmt)))
    if not row:
        raise _lib.PfvError(_lib.PFV_ERR_BAD_ARG, "pixel format must be rgb8, rgba8 or bgra8")
    return int(height), int(width), row // int(width)


def frames_to_rgb(ctx: Context, width: int, height: int, frames, fmt="rgb8") -> np.ndarray:
    """packed Y|U|V 4:2:0 frames (uint8, n frames) as interleaved pictures, uint8 [n, height, width, 3 or 4]: the reference's save_frame
    arithmetic (include/pfv_hip_ext.h, "RGB / RGBA texture output"), fmt "rgb8" / "rgba8" / "bgra8" (pfv_frames_to_rgb)"""
    fb = int(ctx._lib.pfv_frame_bytes(int(width), int(height)))
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    assert fb > 0 and f.size % fb == 0 and f.size
    n = f.size // fb
    m = pix_format(fmt)
    out = np.empty((n,) + rgb_shape(ctx, width, height, m), dtype=np.uint8)
    ctx.check(ctx._lib.pfv_frames_to_rgb(ctx.handle, int(width), int(height), n, ptr(f), ptr(out), m))
    return out


CHROMA_MODES = {"point": _lib.PFV_CHROMA_POINT, "box": _lib.PFV_CHROMA_BOX}


def chroma_mode(chroma) -> int:
    """a chroma mode of the RGB inputs: "point" / "box" or a PFV_CHROMA_* value"""
    return CHROMA_MODES[chroma.lower()] if isinstance(chroma, str) else int(chroma)


def frames_from_rgb(ctx: Context, width: int, height: int, pictures, fmt="rgb8", chroma="point") -> np.ndarray:
    """tight interleaved pictures (uint8, n pictures of [height, width, 3 or 4]) as packed Y|U|V 4:2:0 frames, uint8 [n, frame bytes]: the
    reference's load_frame arithmetic (include/pfv_hip_ext.h, "RGB / RGBA picture input"), fmt "rgb8" / "rgba8" / "bgra8", chroma "point"
    (the reference's: the even pixel's chroma) or "box" (the mean of the 2 x 2 pixels' chroma) (pfv_frames_from_rgb)"""
    fb = int(ctx._lib.pfv_frame_bytes(int(width), int(height)))
    m = pix_format(fmt)
    pic = int(np.prod(rgb_shape(ctx, width, height, m)))
    p = np.ascontiguousarray(pictures, dtype=np.uint8).reshape(-1)
    assert fb > 0 and p.size % pic == 0 and p.size
    n = p.size // pic
    out = np.empty((n, fb), dtype=np.uint8)
    ctx.check(ctx._lib.pfv_frames_from_rgb(ctx.handle, int(width), int(height), n, ptr(p), ptr(out), m, chroma_mode(chroma)))
    return out


class FrameSsimStruct(ctypes.Structure):
    """pfv_frame_ssim"""
    _fields_ = [("q24", ctypes.c_int64 * 3), ("windows", ctypes.c_uint32 * 3), ("ssim", ctypes.c_double * 3), ("ssim_all", ctypes.c_double)]


@dataclass
class FrameSsim:
    """the structural similarity between the frame one ``Encoder.encode_*`` call was given and its reconstruction"""
    q24: tuple            # Y, U, V sums of the windows' values in 2^-24 fixed point; zeros for a drop frame
    windows: tuple        # windows per plane
    ssim: tuple           # per plane
    ssim_all: float       # over all windows of the frame


class FrameReportStruct(ctypes.Structure):
    """pfv_frame_report"""
    _fields_ = [("type", ctypes.c_int32), ("packet_bytes", ctypes.c_uint32), ("sse", ctypes.c_uint64 * 3), ("psnr", ctypes.c_double * 3),
                ("psnr_yuv", ctypes.c_double)]


@dataclass
class FrameReport:
    """what one ``Encoder.encode_*`` call wrote and how far its reconstruction is from the frame it was given"""
    type: int             # 1 i-frame, 2 p-frame, 3 drop frame
    packet_bytes: int     # 5-byte packet header + payload
    sse: tuple            # Y, U, V; zeros for a drop frame
    psnr: tuple           # per plane, dB
    psnr_yuv: float


def session_distortion(session, call, frames, mb_map: bool, out, out_map, sum_dtype=np.uint64, map_dtype=np.uint32):
    """shared body of EncoderSession.distortion / .ssim and DecoderSession.distortion / .ssim: frames (an array -- uploaded -- or a device address) through
    `call` (frames_dev, sse_dev, map_dev); `out` / `out_map` preset the results, so that entries of slots outside the session's window
    come back as they were handed in"""
    ctx = session.ctx
    n, tb = session.n_streams, session.total_blocks
    sse = np.zeros((n, 3), dtype=sum_dtype) if out is None else np.ascontiguousarray(out, dtype=sum_dtype).reshape(n, 3).copy()
    mb = None
    if mb_map:
        mb = np.zeros((n, tb), dtype=map_dtype) if out_map is None else np.ascontiguousarray(out_map, dtype=map_dtype).reshape(n, tb).copy()
    bufs = []
    try:
        if isinstance(frames, (int, np.integer)):
            frames_dev = int(frames)
        else:
            f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
            frames_dev = ctx.alloc(f.nbytes); bufs.append(frames_dev)
            ctx.upload(frames_dev, f)
        sse_dev = ctx.alloc(sse.nbytes); bufs.append(sse_dev)
        ctx.upload(sse_dev, sse)
        map_dev = 0
        if mb_map:
            map_dev = ctx.alloc(mb.nbytes); bufs.append(map_dev)
            ctx.upload(map_dev, mb)
        call(frames_dev, sse_dev, map_dev)
        ctx.download(sse, sse_dev)
        if mb_map:
            ctx.download(mb, map_dev)
    finally:
        for b in bufs:
            ctx.free(b)
    return (sse, mb) if mb_map else sse
