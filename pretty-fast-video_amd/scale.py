"""Frame resize on the device (include/pfv_hip_ext.h, "frame resize"): the filter tables, the plan object :class:`Scaler` and
:func:`frames_scale`.  The pixels come from k_scale (csrc/pfv_scale_kernels.hip); this module only marshals.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .context import Context, ptr

SCALE_KINDS = {"bilinear": _lib.PFV_SCALE_BILINEAR, "bicubic": _lib.PFV_SCALE_BICUBIC, "lanczos3": _lib.PFV_SCALE_LANCZOS3}
_LAYOUTS = {"packed": _lib.PFV_FRAME_PACKED, "padded": _lib.PFV_FRAME_PADDED}


def scale_kind(kind) -> int:
    """a filter kind: "bilinear" / "bicubic" / "lanczos3" or a PFV_SCALE_* value"""
    return SCALE_KINDS[kind.lower()] if isinstance(kind, str) else int(kind)


def scale_taps(kind, n_src: int, n_dst: int) -> int:
    """taps per output sample of one axis; 0 for bad arguments or a reduction beyond 8 (pfv_scale_taps)"""
    return int(_lib.load().pfv_scale_taps(scale_kind(kind), int(n_src), int(n_dst)))


def scale_table(kind, n_src: int, n_dst: int):
    """the table of one axis: (first int32 [n_dst], coef int16 [n_dst, taps]) (pfv_scale_table)"""
    k = scale_kind(kind)
    taps = scale_taps(k, n_src, n_dst)
    if not taps:
        raise _lib.PfvError(_lib.PFV_ERR_BAD_ARG, "scale_table: a kind that does not exist, a size outside 1 .. 65535 or a reduction beyond 8")
    first = np.zeros(int(n_dst), dtype=np.int32)
    coef = np.zeros((int(n_dst), taps), dtype=np.int16)
    _lib.check(None, _lib.load().pfv_scale_table(k, int(n_src), int(n_dst), ptr(first), ptr(coef)))
    return first, coef


class Scaler:
    """pfv_scaler: the four tables of one (source size, destination size, kind) on the device"""

    def __init__(self, ctx: Context, sw: int, sh: int, dw: int, dh: int, kind="bicubic"):
        self.ctx = ctx
        self.src_size, self.dst_size, self.kind = (int(sw), int(sh)), (int(dw), int(dh)), scale_kind(kind)
        err = ctypes.c_int(0)
        self.handle = ctx._lib.pfv_scaler_create(ctx.handle, int(sw), int(sh), int(dw), int(dh), self.kind, ctypes.byref(err))
        if not self.handle:
            self.handle = None
            ctx.check(err.value or _lib.PFV_ERR_BAD_ARG)
        self.src_frame_bytes = int(ctx._lib.pfv_frame_bytes(int(sw), int(sh)))
        self.dst_frame_bytes = int(ctx._lib.pfv_frame_bytes(int(dw), int(dh)))
        ctx._sessions.add(self)              # closed with the context at the latest: it holds device memory of it

    def run_dev(self, n_streams: int, src_dev: int, dst_dev: int, src_layout="packed", src_stride: int = 0, dst_stride: int = 0):
        """asynchronous, one k_scale: n_streams frames at src_dev ("packed" / "padded", src_stride apart; 0: the layout's frame size) into
        packed frames at dst_dev (dst_stride apart; 0: the frame size) (pfv_scaler_run_dev)"""
        layout = _LAYOUTS[src_layout] if isinstance(src_layout, str) else int(src_layout)
        self.ctx.check(self.ctx._lib.pfv_scaler_run_dev(self.handle, int(n_streams), ctypes.c_void_p(src_dev), layout, int(src_stride),
                                                        ctypes.c_void_p(dst_dev), int(dst_stride)))

    def run(self, frames) -> np.ndarray:
        """packed frames (uint8, n frames of the source size) -> uint8 [n, frame bytes of the destination size]; synchronises"""
        f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        assert f.size and f.size % self.src_frame_bytes == 0
        n = f.size // self.src_frame_bytes
        out = np.empty((n, self.dst_frame_bytes), dtype=np.uint8)
        ctx = self.ctx
        s_dev, d_dev = ctx.alloc(f.nbytes), ctx.alloc(out.nbytes)
        try:
            ctx.upload(s_dev, f)
            self.run_dev(n, s_dev, d_dev)
            ctx.download(out, d_dev)
        finally:
            ctx.free(s_dev)
            ctx.free(d_dev)
        return out

    def close(self):
        if self.handle:
            self.ctx._lib.pfv_scaler_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def frames_scale(ctx: Context, sw: int, sh: int, dw: int, dh: int, frames, kind="bicubic") -> np.ndarray:
    """packed Y|U|V 4:2:0 frames (uint8, n frames of sw x sh) resized to dw x dh: uint8 [n, frame bytes]; kind "bilinear" / "bicubic" /
    "lanczos3" (pfv_frames_scale)"""
    sfb, dfb = int(ctx._lib.pfv_frame_bytes(int(sw), int(sh))), int(ctx._lib.pfv_frame_bytes(int(dw), int(dh)))
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    if not sfb or not dfb:
        raise _lib.PfvError(_lib.PFV_ERR_BAD_ARG, "frames_scale: widths and heights must be positive and even")
    assert f.size and f.size % sfb == 0
    n = f.size // sfb
    out = np.empty((n, dfb), dtype=np.uint8)
    ctx.check(ctx._lib.pfv_frames_scale(ctx.handle, int(sw), int(sh), int(dw), int(dh), n, ptr(f), ptr(out), scale_kind(kind)))
    return out
