"""Distortion measured on the device (include/pfv_hip_ext.h, "distortion on the device"): squared error per plane and per
macroblock between frames, PSNR, and the frame report of :class:`Encoder`.  The sums come from the k_sse_* kernels
(csrc/pfv_quality_kernels.hip); this module only marshals.
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


def session_distortion(session, call, frames, mb_map: bool, out, out_map):
    """shared body of EncoderSession.distortion / DecoderSession.distortion: frames (an array -- uploaded -- or a device address) through
    `call` (frames_dev, sse_dev, map_dev); `out` / `out_map` preset the results, so that entries of slots outside the session's window
    come back as they were handed in"""
    ctx = session.ctx
    n, tb = session.n_streams, session.total_blocks
    sse = np.zeros((n, 3), dtype=np.uint64) if out is None else np.ascontiguousarray(out, dtype=np.uint64).reshape(n, 3).copy()
    mb = None
    if mb_map:
        mb = np.zeros((n, tb), dtype=np.uint32) if out_map is None else np.ascontiguousarray(out_map, dtype=np.uint32).reshape(n, tb).copy()
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
