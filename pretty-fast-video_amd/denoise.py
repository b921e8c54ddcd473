"""Denoising pre-filter on the device (include/pfv_hip_ext.h, "denoising pre-filter"): the object :class:`Denoiser`, which owns the streams'
temporal state, and :func:`frames_denoise`.  The samples come from k_denoise (csrc/pfv_denoise_kernels.hip); this module only marshals.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .context import Context, ptr

_LAYOUTS = {"packed": _lib.PFV_FRAME_PACKED, "padded": _lib.PFV_FRAME_PADDED}


def strengths(values) -> np.ndarray:
    """three strengths (Y, U, V) as the uint8[3] the C calls take; one number stands for all three planes"""
    v = np.array([values] * 3 if np.isscalar(values) else list(values), dtype=np.int64)
    if v.shape != (3,) or (v < 0).any() or (v > 255).any():
        raise _lib.PfvError(_lib.PFV_ERR_BAD_ARG, "denoise: three strengths per stage, each 0 .. 16")
    return v.astype(np.uint8)


class Denoiser:
    """pfv_denoiser: the previous output and the primed flag of n_streams streams of width x height"""

    def __init__(self, ctx: Context, width: int, height: int, n_streams: int = 1, spatial=(0, 0, 0), temporal=(0, 0, 0)):
        self.ctx = ctx
        self.width, self.height, self.n_streams = int(width), int(height), int(n_streams)
        err = ctypes.c_int(0)
        self.handle = ctx._lib.pfv_denoiser_create(ctx.handle, self.width, self.height, self.n_streams, ctypes.byref(err))
        if not self.handle:
            self.handle = None
            ctx.check(err.value or _lib.PFV_ERR_BAD_ARG)
        self.frame_bytes = int(ctx._lib.pfv_frame_bytes(self.width, self.height))
        ctx._sessions.add(self)              # closed with the context at the latest: it holds device memory of it
        self.set_strength(spatial, temporal)

    def set_strength(self, spatial, temporal):
        """per plane (Y, U, V), 0 .. 16, for the runs that follow (pfv_denoiser_set_strength)"""
        s, t = strengths(spatial), strengths(temporal)
        self.ctx.check(self.ctx._lib.pfv_denoiser_set_strength(self.handle, ptr(s), ptr(t)))

    def reset(self, first_stream: int = 0, n: int | None = None):
        """un-primes streams [first_stream, first_stream + n): their next frame is filtered spatially only (pfv_denoiser_reset)"""
        self.ctx.check(self.ctx._lib.pfv_denoiser_reset(self.handle, int(first_stream), int(self.n_streams - first_stream if n is None else n)))

    def run_dev(self, src_dev: int, dst_dev: int, first_stream: int = 0, n: int | None = None, src_layout="packed", src_stride: int = 0,
                dst_stride: int = 0, commit: bool = True):
        """asynchronous, one k_denoise: the frames of streams [first_stream, first_stream + n) at src_dev ("packed" / "padded", src_stride
        apart; 0: the layout's frame size) into packed frames at dst_dev (dst_stride apart; 0: the frame size); commit: the output also
        becomes the streams' state (pfv_denoiser_run_dev)"""
        layout = _LAYOUTS[src_layout] if isinstance(src_layout, str) else int(src_layout)
        self.ctx.check(self.ctx._lib.pfv_denoiser_run_dev(self.handle, int(first_stream), int(self.n_streams - first_stream if n is None else n),
                                                          ctypes.c_void_p(src_dev), layout, int(src_stride), ctypes.c_void_p(dst_dev), int(dst_stride),
                                                          1 if commit else 0))

    def run(self, frames, commit: bool = True) -> np.ndarray:
        """one packed frame per stream (uint8 [n_streams, frame bytes]) -> the filtered frames; synchronises"""
        f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        assert f.size == self.n_streams * self.frame_bytes
        out = np.empty((self.n_streams, self.frame_bytes), dtype=np.uint8)
        ctx = self.ctx
        s_dev, d_dev = ctx.alloc(f.nbytes), ctx.alloc(out.nbytes)
        try:
            ctx.upload(s_dev, f)
            self.run_dev(s_dev, d_dev, commit=commit)
            ctx.download(out, d_dev)
        finally:
            ctx.free(s_dev)
            ctx.free(d_dev)
        return out

    def close(self):
        if self.handle:
            self.ctx._lib.pfv_denoiser_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def frames_denoise(ctx: Context, width: int, height: int, frames, spatial, temporal, n_streams: int = 1) -> np.ndarray:
    """packed Y|U|V 4:2:0 frames (uint8, frame-major: [frame][stream]) through a fresh filter, in order: uint8 [n_frames * n_streams, frame
    bytes] (pfv_frames_denoise)"""
    fb = int(ctx._lib.pfv_frame_bytes(int(width), int(height)))
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    if not fb:
        raise _lib.PfvError(_lib.PFV_ERR_BAD_ARG, "frames_denoise: width and height must be positive and even")
    assert f.size and f.size % (fb * int(n_streams)) == 0
    n_frames = f.size // (fb * int(n_streams))
    out = np.empty((n_frames * int(n_streams), fb), dtype=np.uint8)
    s, t = strengths(spatial), strengths(temporal)
    ctx.check(ctx._lib.pfv_frames_denoise(ctx.handle, int(width), int(height), int(n_streams), n_frames, ptr(f), ptr(out), ptr(s), ptr(t)))
    return out
