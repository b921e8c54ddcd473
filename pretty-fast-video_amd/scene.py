"""Scene-cut detection on the device (include/pfv_hip_ext.h, "scene-cut detection"): the object :class:`SceneDetector`, which owns the
streams' previous quarter planes, :func:`frames_scene`, and the pure host functions :func:`scene_score` and :func:`scene_plan`.  The numbers
come from k_scene_quarter / k_scene_cost / k_scene_sum (csrc/pfv_scene_kernels.hip); this module only marshals.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from .context import Context, ptr

_LAYOUTS = {"packed": _lib.PFV_FRAME_PACKED, "padded": _lib.PFV_FRAME_PADDED}
RADIUS_DEFAULT = 4          # PFV_SCENE_RADIUS_DEFAULT
THRESHOLD_DEFAULT = 176     # PFV_SCENE_THRESHOLD_DEFAULT
# pfv_scene_stats, 40 bytes
STATS_DTYPE = np.dtype([("inter", "<u8"), ("intra", "<u8"), ("zero", "<u8"), ("n_blocks", "<u4"), ("n_intra", "<u4"), ("n_moving", "<u4"), ("reserved", "<u4")])
assert STATS_DTYPE.itemsize == 40


class SceneStats(NamedTuple):
    """pfv_scene_stats of one pair of frames"""
    inter: int
    intra: int
    zero: int
    n_blocks: int
    n_intra: int
    n_moving: int
    reserved: int = 0

    @classmethod
    def from_record(cls, r) -> "SceneStats":
        return cls(*(int(r[k]) for k in STATS_DTYPE.names))

    @property
    def score(self) -> int:
        return scene_score(self)


def stats_array(stats) -> np.ndarray:
    """SceneStats, a sequence of them or a structured array -> a contiguous STATS_DTYPE array"""
    if isinstance(stats, np.ndarray) and stats.dtype == STATS_DTYPE:
        return np.ascontiguousarray(stats).reshape(-1)
    if isinstance(stats, (SceneStats, np.void)):      # one pair: the tuple, or one record of a structured array
        stats = [stats]
    return np.array([tuple(s) for s in stats], dtype=STATS_DTYPE)


def scene_score(stats) -> int:
    """the score in q8 of one pair: 0 without a previous frame, else min(65535, inter * 256 // max(intra, 64 * n_blocks)) (pfv_scene_score_q8)"""
    a = stats_array(stats)
    assert a.size == 1
    return int(_lib.load().pfv_scene_score_q8(ptr(a)))


def scene_plan(stats, threshold_q8: int = THRESHOLD_DEFAULT, min_interval: int = 0, max_interval: int = 0) -> np.ndarray:
    """frame types (1 i-frame, 2 p-frame) for the frames the stats describe, in order (pfv_scene_plan)"""
    a = stats_array(stats)
    types = np.zeros(a.size, dtype=np.uint8)
    rc = int(_lib.load().pfv_scene_plan(ptr(a), int(a.size), int(threshold_q8), int(min_interval), int(max_interval), ptr(types)))
    if rc < 0:
        raise _lib.PfvError(rc, "scene_plan: bad argument")
    return types


class SceneDetector:
    """pfv_scene_detector: the previous quarter plane and the primed flag of n_streams streams of width x height"""

    def __init__(self, ctx: Context, width: int, height: int, n_streams: int = 1, max_clip_frames: int = 0, radius: int = RADIUS_DEFAULT):
        self.ctx = ctx
        self.width, self.height, self.n_streams, self.max_clip_frames = int(width), int(height), int(n_streams), int(max_clip_frames)
        err = ctypes.c_int(0)
        self.handle = ctx._lib.pfv_scene_detector_create(ctx.handle, self.width, self.height, self.n_streams, self.max_clip_frames, ctypes.byref(err))
        if not self.handle:
            self.handle = None
            ctx.check(err.value or _lib.PFV_ERR_BAD_ARG)
        self.frame_bytes = int(ctx._lib.pfv_frame_bytes(self.width, self.height))
        self.blocks_x, self.blocks_y = (self.width >> 2) >> 3, (self.height >> 2) >> 3
        self.n_blocks = self.blocks_x * self.blocks_y
        ctx._sessions.add(self)              # closed with the context at the latest: it holds device memory of it
        self.set_radius(radius)

    def set_radius(self, radius: int):
        """R in quarter samples, 0 .. 7, for the runs that follow (pfv_scene_detector_set_radius)"""
        self.ctx.check(self.ctx._lib.pfv_scene_detector_set_radius(self.handle, int(radius)))

    def reset(self, first_stream: int = 0, n: int | None = None):
        """un-primes streams [first_stream, first_stream + n): their next frame has no previous one (pfv_scene_detector_reset)"""
        self.ctx.check(self.ctx._lib.pfv_scene_detector_reset(self.handle, int(first_stream), int(self.n_streams - first_stream if n is None else n)))

    def run_dev(self, src_dev: int, stats_dev: int, first_stream: int = 0, n: int | None = None, src_layout="packed", src_stride: int = 0, commit: bool = True):
        """asynchronous, one launch group: the frames of streams [first_stream, first_stream + n) at src_dev ("packed" / "padded", src_stride
        apart; 0: the layout's frame size) against the streams' state into n pfv_scene_stats at stats_dev (pfv_scene_detector_run_dev)"""
        layout = _LAYOUTS[src_layout] if isinstance(src_layout, str) else int(src_layout)
        self.ctx.check(self.ctx._lib.pfv_scene_detector_run_dev(self.handle, int(first_stream), int(self.n_streams - first_stream if n is None else n),
                                                                ctypes.c_void_p(src_dev), layout, int(src_stride), 1 if commit else 0, ctypes.c_void_p(stats_dev)))

    def run_clip_dev(self, frames_dev: int, n_frames: int, stats_dev: int, stream: int = 0, layout="packed", stride: int = 0, commit: bool = True):
        """asynchronous, one launch group: n_frames consecutive frames of ONE stream, the first against the stream's state, frame k against
        frame k - 1 (pfv_scene_detector_run_clip_dev)"""
        lay = _LAYOUTS[layout] if isinstance(layout, str) else int(layout)
        self.ctx.check(self.ctx._lib.pfv_scene_detector_run_clip_dev(self.handle, int(stream), int(n_frames), ctypes.c_void_p(frames_dev), lay, int(stride),
                                                                     1 if commit else 0, ctypes.c_void_p(stats_dev)))

    def run_timed_dev(self, src_dev: int, n: int, stats_dev: int, first: int = 0, clip: bool = False, layout="packed", stride: int = 0):
        """measurement only: an uncommitted run_dev (or, clip: run_clip_dev on stream `first`) with events between the kernels -> milliseconds of
        (k_scene_quarter, k_scene_cost, k_scene_sum); synchronises (pfv_scene_detector_run_timed_dev)"""
        lay = _LAYOUTS[layout] if isinstance(layout, str) else int(layout)
        ms = (ctypes.c_float * 3)()
        self.ctx.check(self.ctx._lib.pfv_scene_detector_run_timed_dev(self.handle, int(first), int(n), 1 if clip else 0, ctypes.c_void_p(src_dev), lay, int(stride),
                                                                      ctypes.c_void_p(stats_dev), ms))
        return tuple(float(v) for v in ms)

    def _host(self, frames, n: int, call) -> np.ndarray:
        f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        assert f.size == n * self.frame_bytes
        out = np.zeros(n, dtype=STATS_DTYPE)
        ctx = self.ctx
        s_dev, d_dev = ctx.alloc(f.nbytes), ctx.alloc(out.nbytes)
        try:
            ctx.upload(s_dev, f)
            call(s_dev, d_dev)
            ctx.download(out, d_dev)
        finally:
            ctx.free(s_dev)
            ctx.free(d_dev)
        return out

    def run(self, frames, commit: bool = True) -> np.ndarray:
        """one packed frame per stream (uint8 [n_streams, frame bytes]) -> STATS_DTYPE [n_streams]; synchronises"""
        return self._host(frames, self.n_streams, lambda s, d: self.run_dev(s, d, commit=commit))

    def run_clip(self, frames, stream: int = 0, commit: bool = True) -> np.ndarray:
        """consecutive packed frames of one stream (uint8 [n_frames, frame bytes]) -> STATS_DTYPE [n_frames]; synchronises"""
        n = np.asarray(frames).reshape(-1).size // self.frame_bytes
        return self._host(frames, n, lambda s, d: self.run_clip_dev(s, n, d, stream=stream, commit=commit))

    def maps(self, first: int = 0, n: int = 1):
        """the block maps of the last run, entries [first, first + n): (uint32 [n, blocks_y, blocks_x] = best << 16 | intra,
        int8 [n, blocks_y, blocks_x, 2] = the chosen (cx, cy)); waits for the stream (pfv_scene_detector_maps)"""
        blk = np.zeros((n, self.blocks_y, self.blocks_x), dtype=np.uint32)
        vec = np.zeros((n, self.blocks_y, self.blocks_x, 2), dtype=np.int8)
        self.ctx.check(self.ctx._lib.pfv_scene_detector_maps(self.handle, int(first), int(n), ptr(blk), ptr(vec)))
        return blk, vec

    def close(self):
        if self.handle:
            self.ctx._lib.pfv_scene_detector_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def frames_scene(ctx: Context, width: int, height: int, frames, radius: int = RADIUS_DEFAULT, n_streams: int = 1) -> np.ndarray:
    """packed Y|U|V 4:2:0 frames (uint8, frame-major: [frame][stream]) through a fresh detector, in order: STATS_DTYPE [n_frames, n_streams]
    (pfv_frames_scene)"""
    fb = int(ctx._lib.pfv_frame_bytes(int(width), int(height)))
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    if not fb:
        raise _lib.PfvError(_lib.PFV_ERR_BAD_ARG, "frames_scene: width and height must be positive and even")
    assert f.size and f.size % (fb * int(n_streams)) == 0
    n_frames = f.size // (fb * int(n_streams))
    out = np.zeros((n_frames, int(n_streams)), dtype=STATS_DTYPE)
    ctx.check(ctx._lib.pfv_frames_scene(ctx.handle, int(width), int(height), int(n_streams), n_frames, ptr(f), int(radius), ptr(out)))
    return out
